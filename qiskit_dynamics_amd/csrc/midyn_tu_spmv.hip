// midyn_tu_spmv.hip -- translation unit of libmidyn.so that holds the gather kernels of the sparse-operator route (spmv_cols_kernel,
// spmv_rows_kernel, spmv_prep_kernel, spmv_load_kernel)
// (list: the extern-template block at the end of midyn_spmv.h; host side: midyn_spmv.inc in midyn.hip).
#define MIDYN_FAMILY_TU 1
#define MIDYN_TU_SPMV 1
#include <hip/hip_runtime.h>

#include "midyn_spmv.h"
