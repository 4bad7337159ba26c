// Test probe for mc-alf_amd/csrc/voigt_grad.h (tests/test_gpu_voigt_grad.py): every output of faddeeva_dw and of faddeeva_d2w
// at n points, eleven doubles per point, [wr, wi, dr, di, e | wr, dr, e, d2, e2, e3].  Built by the tests with the flags of
// grad_kernels.o; it is no part of the product library.
#include <hip/hip_runtime.h>

#include "voigt_grad.h"

__global__ void voigt_grad_probe_kernel(const double* x, const double* y, long n, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double* o = out + 11 * i;
    mcalf::faddeeva_dw(x[i], y[i], o[0], o[1], o[2], o[3], o[4]);
    mcalf::faddeeva_d2w(x[i], y[i], o[5], o[6], o[7], o[8], o[9], o[10]);
}

// out: 11 n doubles.  Returns the first HIP error (0: none).
extern "C" int voigt_grad_probe(const double* x, const double* y, long n, double* out) {
    if (n <= 0) return 0;
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    hipError_t e = hipMalloc((void**)&dx, nb);
    if (e == hipSuccess) e = hipMalloc((void**)&dy, nb);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, 11 * nb);
    if (e == hipSuccess) e = hipMemcpy(dx, x, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        voigt_grad_probe_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(dx, dy, n, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, 11 * nb, hipMemcpyDeviceToHost);
    for (double* b : {dx, dy, dout})
        if (b) (void)hipFree(b);
    return (int)e;
}
