// Version entry points of libxai_ext.so (include/xai_hip_ext.h).  Error texts stay with xai_strerror in libxai_hip.so.
#include "xai_common.h"
#include "xai_hip_ext.h"

XAI_EXPORT int xai_ext_version(void) { return XAI_EXT_VERSION; }
XAI_EXPORT int xai_ext_version_minor(void) { return XAI_EXT_MINOR; }
