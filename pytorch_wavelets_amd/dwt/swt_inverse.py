"""``pytorch_wavelets.dwt.swt_inverse``'s import path: the inverse stationary transform and its function-level banks (the
implementations live with the other transforms, in transform2d.py and lowlevel.py)."""
from .lowlevel import sfb1d_atrous, sfb2d_atrous
from .transform2d import SWTInverse

__all__ = ['SWTInverse', 'sfb1d_atrous', 'sfb2d_atrous']
