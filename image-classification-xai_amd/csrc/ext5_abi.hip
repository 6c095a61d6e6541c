// Version entry points of libxai_ext5.so (include/xai_hip_ext5.h); its kernels are in quickshift_kernels.hip (K53-K55).  Error texts
// stay with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext5.h"

XAI_EXPORT int xai_ext5_version(void) { return XAI_EXT5_VERSION; }
XAI_EXPORT int xai_ext5_version_minor(void) { return XAI_EXT5_MINOR; }
