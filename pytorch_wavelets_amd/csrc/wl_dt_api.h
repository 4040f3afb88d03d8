// What the translation units of the DTCWT / ScatLayer C ABI (wl_api.inc, wl_strip_api.inc, wl_dtinv_api.inc) share on the host
// side, declared once.  No kernel header is pulled in: the argument structs are forward declarations (wl_dtcwt_kernels.h).
#pragma once
#include "../../include/wavelets_hip.h"

int wl_streaming_off();   // wl_api.inc: 1 when the streaming kernels are switched off (generic_only / no_stream)

template <typename T> struct WlDtFwd1Args;
template <typename T> struct WlDtFwd2Args;
template <typename T> struct WlDtInv1Args;
template <typename T> struct WlDtInv2Args;

// The streaming kernels the per-level launchers of wl_api.inc try first.  Defined in wl_strip_api.inc (part 4), which instantiates
// them for float32, float16 and bfloat16; WL_ERR_UNSUPPORTED = not this kernel's case, the caller goes on to the tile kernels.
template <typename T> int wl_dtfwd1_strip(const WlDtFwd1Args<T>& f, void* stream);    // level-1 forward over column strips (wl_dtcwt_strip.h)
template <typename T> int wl_dtfwd1_lean(const WlDtFwd1Args<T>& f, void* stream);     // lean level-1 / ScatLayer strip kernels (wl_dtcwt_fused.h)
template <typename T> int wl_dtrot_lean(const WlDtFwd1Args<T>& f, const void* h2, int L2, void* stream);   // ... with the band-pass diagonal (MODE 6)
template <typename T> int wl_dtfwd2_lean(const WlDtFwd2Args<T>& g, void* stream);     // streaming level >= 2 forward (wl_dtcwt_fused.h MODE 4)
template <typename T> int wl_dtinv2_strip(const WlDtInv2Args<T>& f, void* stream);    // streaming level >= 2 inverse (wl_dtcwt_fused.h)
template <typename T> int wl_dtinv1_strip(const WlDtInv1Args<T>& f, void* stream);    // level-1 inverse / ScatLayer backward over column strips
// float64 has no streaming kernel
template <> inline int wl_dtfwd1_strip<double>(const WlDtFwd1Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
template <> inline int wl_dtfwd1_lean<double>(const WlDtFwd1Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
template <> inline int wl_dtrot_lean<double>(const WlDtFwd1Args<double>&, const void*, int, void*) { return WL_ERR_UNSUPPORTED; }
template <> inline int wl_dtfwd2_lean<double>(const WlDtFwd2Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
template <> inline int wl_dtinv2_strip<double>(const WlDtInv2Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
template <> inline int wl_dtinv1_strip<double>(const WlDtInv1Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
