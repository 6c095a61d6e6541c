// Version entry points of libxai_ext6.so (include/xai_hip_ext6.h); its kernels are in linkage_kernels.hip (K56-K57).  Error texts
// stay with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext6.h"

XAI_EXPORT int xai_ext6_version(void) { return XAI_EXT6_VERSION; }
XAI_EXPORT int xai_ext6_version_minor(void) { return XAI_EXT6_MINOR; }
