// What the optical-depth kinematics kernels (kin_kernels.hip) and their host side (host_kin.cpp) share: the argument block, the
// workspace layout and the kernel handles.  Plain C++ -- host_kin.cpp is compiled without the HIP language mode.
// Not part of the kernel-source hash (mc-alf_amd/build.py): the fused kernel does not include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "eqw_args.h"

namespace mcalf {

// The pixel kernels walk a spectrum exactly as the equivalent widths' pixel kernel does (eqw_args.h): pixel j of thread t of
// tile T is T * kKinTile + j * kKinBlock + t.  A SLAB is the 64 consecutive pixels one wave holds at one j: slab j * kKinWaves +
// w of the tile, so slabs are numbered in pixel order, kKinSlabs per tile.
constexpr int kKinBlock = kEqwBlock, kKinPpt = kEqwPpt, kKinTile = kEqwTile, kKinWaves = kEqwWaves;
constexpr int kKinSlabs = kKinPpt * kKinWaves;    // 32 slabs per tile
constexpr int kKinMaxQ = 16;                      // quantiles per call
constexpr int kKinHead = 2 + kKinMaxQ;            // doubles per (row, line) head: I, lam_mean, the nq targets q[j] I
constexpr int kKinCand = 3;                       // doubles per quantile candidate: pixel k (-1: none), S[k], t[k]

// One pass over `nrows` rows of a batch.  The records are the equivalent widths' (mcalf_eqw_setup_kernel under
// kEqwIndexLayout writes them: the same count, the same columns, the same kinds).
struct KinArgs {
    const double *nu, *dlam;  // [npix] pixel frequency at z = 0; wavelength step (the context's arrays of eqw_args.h)
    const double *wl, *edge;  // [npix] wavelength; [npix + 1] cell edges (host_kin.cpp: kin_prepare)
    const double* tabs;       // T[VT_NY][VT_NTOT]
    const double* recs;       // [nrows, ncompmax * nlines, kEqwRec], slot-major
    double* part;             // [nrows, nlines, 2, nslabs], nslabs = ntiles * kKinSlabs.  Plane 0: a slab's sum of t after the sums
                              //   pass, its exclusive offset after finalize A.  Plane 1, its first ntiles * kKinWaves entries: a wave's
                              //   sum of t (wl - piv) after the sums pass, of t (wl - lam_mean)^2 after the scan pass.
    double* head;             // [nrows, nlines, kKinHead]
    double* cand;             // [nrows, nlines, ntiles * kKinWaves, nq, kKinCand]: per wave its first pixel with !(S < target)
    double* mom;              // [nrows, nlines, 3] or nullptr: I, lam_mean, lam_rms
    double* lamq;             // [nrows, nlines, nq] or nullptr
    int nrows, npix, ntiles, nq;
    RowLayout lay;            // how a row of P is read (theta_row.h); the pixel kernels take ncompmax and nlines from it
    double q[kKinMaxQ];
};

// The kernels of kin_kernels.hip; all take (const KinArgs a).
enum KinKernel {
    kKinSums,         // grid = (ntiles, nrows), kKinBlock threads: the Voigt pass, per slab the sum of t, per wave that of t (wl - piv)
    kKinOffsets,      // grid = ceil(nrows * nlines / 64), 64 threads ("finalize A"): the slabs' exclusive offsets in pixel order, I, lam_mean, targets
    kKinScan,         // grid = (ntiles, nrows), kKinBlock threads: the Voigt pass again, S per pixel, the candidates, the centred squares
    kKinFinalize,     // grid = ceil(nrows * nlines / 64), 64 threads ("finalize B"): the first candidate per quantile, interpolation, lam_rms, the NaN rules
    kKinKernelCount
};
MCALF_INTERNAL const void* kin_kernel_ptr(KinKernel k);

}  // namespace mcalf
