// The kernels of the ragged large-fold leave-fold-out predictives (blr_kfold_large_ragged.hpp) instantiated in a translation unit of
// their own.  Host side: blr_abi.hip (kfold_large_ragged).
#include <hip/hip_runtime.h>

#include "blr_kfold_large_ragged.hpp"

namespace blr {

BLR_KFLR_ALL(template)

}  // namespace blr
