// Version entry points of libxai_ext3.so (include/xai_hip_ext3.h); its kernels are in seg_kernels.hip (K44-K45).  Error texts stay
// with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext3.h"

XAI_EXPORT int xai_ext3_version(void) { return XAI_EXT3_VERSION; }
XAI_EXPORT int xai_ext3_version_minor(void) { return XAI_EXT3_MINOR; }
