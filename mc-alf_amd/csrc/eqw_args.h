// What the equivalent-width kernels (eqw_kernels.hip) and their host side (host_eqw.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_eqw.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernel_args.h"
#include "theta_row.h"

namespace mcalf {

constexpr int kEqwBlock = 256;                    // threads per workgroup of the pixel kernel (four waves)
constexpr int kEqwPpt = 8;                        // pixels per thread: pixel j of thread t is tile0 + j * kEqwBlock + t
constexpr int kEqwTile = kEqwBlock * kEqwPpt;     // 2048 pixels per workgroup: a line's fold (2 coefficients per thread) is
                                                  // paid once per 8 pixel evaluations of every thread
constexpr int kEqwWaves = kEqwBlock / 64;
constexpr int kEqwRec = 8;                        // doubles per (slot, line) record: A, B, y, K, K y / sqrt(pi), kind, 1 + z, (pad)
constexpr int kEqwIndexLayout = 0, kEqwIndexAsWritten = 1;   // MCALF_EQW_LAYOUT / MCALF_EQW_AS_WRITTEN of the C ABI
// a record's kind: how the pixel kernel evaluates it
constexpr double kEqwInactive = 0.0;              // layout mode, slot at or beyond the row's active count: cell exactly 0, parameters never read
constexpr double kEqwFast = kRecFast;             // the y-folded tables
constexpr double kEqwGeneral = kRecGeneral;       // hjert_general: a outside [0, 2^-8], absurd columns
constexpr double kEqwZero = kRecZero;             // |1 + z| beyond 1e100: every |u| overflows, tau = 0 (theta_row.h: record_kind)

// One pass over `nrows` rows of a batch.
struct EqwArgs {
    const double* P;          // parameter rows of this pass, row-major [nrows, ndim]
    const double *nu, *dlam;  // [npix] pixel frequency at z = 0; wavelength step (hires_fitter.py:485-486)
    const LineDev* lines;     // nlines target lines
    const double* tabs;       // T[VT_NY][VT_NTOT]
    double* recs;             // [nrows, ncompmax * nlines, kEqwRec], slot-major
    double* part;             // [nrows, ntiles, ncells, kEqwWaves] per-wave partial sums; ncells = (ncompmax + 1) * nlines:
                              //   cell c * nlines + l = component c, line l; cell ncompmax * nlines + l = the blend of line l
    double* Wcomp;            // [nrows, ncompmax, nlines] or nullptr
    double* Wblend;           // [nrows, nlines] or nullptr
    int nrows, npix, ntiles, indexing;
    RowLayout lay;            // how a row of P is read (theta_row.h)
};

// The kernels of eqw_kernels.hip; all take (const EqwArgs a).
enum EqwKernel {
    kEqwSetup,        // grid = nrows, 64 threads: decode the slots under a.indexing, one record per (slot, line)
    kEqwPixel,        // grid = (ntiles, nrows), kEqwBlock threads: the Voigt pass and the per-wave sums
    kEqwFinalize,     // grid = ceil(nrows * ncells / 256), 256 threads: tiles and waves summed in order, / (1 + z)
    kEqwKernelCount
};
MCALF_INTERNAL const void* eqw_kernel_ptr(EqwKernel k);

}  // namespace mcalf
