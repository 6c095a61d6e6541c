// Version entry points of libxai_ext2.so (include/xai_hip_ext2.h); its kernels are in mda_kernels.hip (K36-K38) and
// sanity_kernels.hip (K39-K43).  Error texts stay with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext2.h"

XAI_EXPORT int xai_ext2_version(void) { return XAI_EXT2_VERSION; }
XAI_EXPORT int xai_ext2_version_minor(void) { return XAI_EXT2_MINOR; }
