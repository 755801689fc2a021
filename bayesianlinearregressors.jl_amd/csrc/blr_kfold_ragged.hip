// The kernels of the ragged leave-fold-out predictives (blr_kfold_ragged.hpp) instantiated in a translation unit of their own: the
// code objects of the existing kernels stay as they are.  Host side: blr_abi.hip (kfold_ragged).
#include <hip/hip_runtime.h>

#include "blr_kfold_ragged.hpp"

namespace blr {

BLR_KFOLD_RAGGED_INSTANCES(template, double)
BLR_KFOLD_RAGGED_INSTANCES(template, float)

}  // namespace blr
