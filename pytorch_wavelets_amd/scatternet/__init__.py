from .layers import ScatLayer, ScatLayer1D, ScatLayerj2   # noqa: F401
