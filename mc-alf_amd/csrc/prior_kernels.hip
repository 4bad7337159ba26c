// Device side of mcalf_lnprior_batch[_device], for gfx950: lnprior of a batch of parameter rows or unit-cube rows under the
// context's box and Gaussian factors.  ONE wave64 per row; the arithmetic is row_lnprior's (prior_device.h), which the samplers'
// kernels call on the rows they hold -- so this entry returns the bits their accept rules saw.
#include <hip/hip_runtime.h>

#include "prior_args.h"

#pragma clang fp contract(off)

#include "prior_device.h"

using namespace mcalf;

__global__ __launch_bounds__(kPriorWave) void mcalf_lnprior_kernel(const PriorArgs a) {
    const size_t row = blockIdx.x;
    const double v = row_lnprior(a.prior, a.rows + row * (size_t)a.prior.ndim, a.from_cube);
    if (threadIdx.x == 0) a.out[row] = v;
}

namespace mcalf {
const void* prior_kernel_ptr() { return (const void*)&mcalf_lnprior_kernel; }
}  // namespace mcalf
