// midyn_tu_combine_mirror.hip -- translation unit of libmidyn.so that instantiates the mirrored COMBINE + APPLY kernels (combine_mirror_kernel, mirror_finish_kernel)
// (list: the extern-template block at the end of the kernel header; host side: midyn.hip).
#define MIDYN_FAMILY_TU 1
#define MIDYN_TU_COMBINE_MIRROR 1
#include <hip/hip_runtime.h>

#include "../../include/midyn.h"
#include "midyn_kernels.h"
#include "midyn_combine.h"
#include "midyn_combine_mirror.h"
