// Version entry points of libxai_ext4.so (include/xai_hip_ext4.h); its kernels are in lrp_kernels.hip (K46-K52).  Error texts stay
// with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext4.h"

XAI_EXPORT int xai_ext4_version(void) { return XAI_EXT4_VERSION; }
XAI_EXPORT int xai_ext4_version_minor(void) { return XAI_EXT4_MINOR; }
