// tests/test_theta_row_host.py: the rules by which a parameter row is read (mc-alf_amd/csrc/theta_row.h, the header the
// derivative, equivalent-width and fit kernels decode their rows with), run on the CPU for fixed lists of cases.  One JSON
// record per line: the inputs and what the header gives; doubles that compare by bits are printed as 16 hex digits, other
// doubles as hex floats.  The test computes every expectation itself.  Built with -ffp-contract=off under AddressSanitizer
// and UBSan.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ctx_plan.h"
#include "theta_row.h"

using namespace mcalf;

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// The layout of a context with these counts, from the planner's shape (what host_ctx.h: row_layout does with the context's).
static RowLayout layout_of(int freespecres, int freecont, int nfill, int ncompmax, int jax, CtxShape* shape) {
    const long npix = 96;
    std::vector<double> wl(npix), flux(npix, 1.0), err(npix, 0.05);
    for (long i = 0; i < npix; ++i) wl[i] = 6190.0 * std::exp((double)i * 2.0 / 2.99792458e5);
    mcalf_line lines[2] = {{1548.204, 0.1899, 2.643e8}, {1550.781, 0.09475, 2.628e8}};
    mcalf_spec sp = {};
    sp.npix = npix; sp.wl = wl.data(); sp.flux = flux.data(); sp.err = err.data();
    sp.velstep = 2.0; sp.nlines = 2; sp.lines = lines; sp.fill = mcalf_line{250.0, 0.1899, 2.643e8};
    sp.ncompmax = ncompmax; sp.nfill = nfill; sp.freespecres = freespecres; sp.freecont = freecont;
    sp.specres_fixed = 7.0; sp.specres_max = 8.0; sp.contval_fixed = 0.97;
    sp.conv_mode = jax ? MCALF_CONV_SAME_EDGE_JAX : MCALF_CONV_WRAP_NUMPY; sp.device = -1;
    std::string msg;
    if (check_spec(&sp, &msg) != MCALF_OK || plan_shape(sp, -1, shape, &msg) != MCALF_OK) {
        std::fprintf(stderr, "the planner refused a layout case: %s\n", msg.c_str());
        std::exit(1);
    }
    const CtxShape& s = *shape;
    return {s.ndim, s.nlines, s.ncompmax, s.nfill, s.startind, s.endind, s.freespecres, s.freecont,
            s.conv_mode == MCALF_CONV_SAME_EDGE_JAX ? 1 : 0, s.specres_fixed, s.contval_fixed};
}

static void layouts() {
    for (int fs = 0; fs < 2; ++fs)
        for (int fc = 0; fc < 2; ++fc)
            for (int nfill : {0, 2})
                for (int ncompmax : {1, 3}) {
                    CtxShape s;
                    const RowLayout lay = layout_of(fs, fc, nfill, ncompmax, 0, &s);
                    std::printf("{\"kind\": \"layout\", \"freespecres\": %d, \"freecont\": %d, \"nfill\": %d, \"ncompmax\": %d, \"nlines\": %d, "
                                "\"plan\": {\"ndim\": %d, \"startind\": %d, \"endind\": %d}, \"ndim\": %d, \"startind\": %d, \"endind\": %d, \"cont_col\": %d, "
                                "\"target_col\": [", fs, fc, nfill, ncompmax, lay.nlines, s.ndim, s.startind, s.endind, lay.ndim, lay.startind,
                                lay.endind, cont_col(lay));
                    for (int c = 0; c < ncompmax; ++c) std::printf("%s%d", c ? ", " : "", target_col(lay, c));
                    std::printf("], \"filler_col\": [");
                    for (int k = 0; k < nfill; ++k) std::printf("%s%d", k ? ", " : "", filler_col(lay, k));
                    // a row that carries its own column numbers: R and the continuum read from it, or the fixed values
                    std::vector<double> p(lay.ndim);
                    for (int i = 0; i < lay.ndim; ++i) p[i] = 100.0 + i;
                    std::printf("], \"R\": \"%a\", \"cont\": \"%a\", \"movable\": [", row_resolution(lay, p.data()), row_continuum(lay, p.data()));
                    for (int nc = 0; nc <= ncompmax; ++nc) {
                        std::printf("%s[", nc ? ", " : "");
                        for (int k = 0; k < lay.ndim; ++k) std::printf("%s%d", k ? ", " : "", coord_movable(lay, nc, k) ? 1 : 0);
                        std::printf("]");
                    }
                    std::printf("]}\n");
                }
}

static void counts() {
    const double inf = std::numeric_limits<double>::infinity();
    for (int jax = 0; jax < 2; ++jax)
        for (int ncompmax : {1, 3}) {
            CtxShape s;
            const RowLayout lay = layout_of(1, 1, 1, ncompmax, jax, &s);
            const double m = (double)ncompmax;
            const double values[] = {-inf, -1.5, -0.5, -0.0, 0.0, std::nextafter(1.0, 0.0), 1.0, 1.5, m - 0.5, m, m + 0.5, 1e300, inf, std::nan("")};
            for (double v : values)
                std::printf("{\"kind\": \"count\", \"jax\": %d, \"ncompmax\": %d, \"value\": \"%a\", \"count\": %d}\n", jax, ncompmax, v,
                            active_components(lay, v));
        }
}

static void line_scales() {
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const LineDev civ = {1548.204e-8, 0.1899, 2.643e8 / (4.0 * M_PI), kCcgs / 1548.204e-8};
    const LineDev lya = {1215.67e-8, 0.4164, 6.265e8 / (4.0 * M_PI), kCcgs / 1215.67e-8};
    const LineDev nanline = {nan, 0.1899, 2.643e8 / (4.0 * M_PI), kCcgs / 1548.204e-8};
    const LineDev strong = {1548.204e-8, 0.1899, 3.0e12, kCcgs / 1548.204e-8};          // a far above 2^-8
    struct Case { double z, b; LineDev ln; double cold; };
    // (volatile: the arithmetic below runs at run time, as it does in the kernels)
    static volatile Case cases[] = {
        {3.0, 12.0, civ, 2.5e13},    {2.9991, 3.5, lya, 1.0e14},   {0.0, 40.0, civ, 1.0e12},      {3.0, -12.0, civ, 2.5e13},
        {3.0, 0.0, civ, 2.5e13},     {-1.0, 12.0, civ, 2.5e13},    {1e101, 12.0, civ, 2.5e13},    {-1e101, 12.0, lya, 2.5e13},
        {inf, 12.0, civ, 2.5e13},    {nan, 12.0, civ, 2.5e13},     {3.0, nan, civ, 2.5e13},       {3.0, 12.0, nanline, 2.5e13},
        {3.0, 12.0, civ, nan},       {3.0, 12.0, civ, 1.0e40},     {3.0, 12.0, strong, 2.5e13},   {3.0, 1e-3, civ, 0.0},
    };
    for (volatile Case& vc : cases) {
        const double z = vc.z, b = vc.b, cold = vc.cold;
        const LineDev ln = {vc.ln.wrest_cm, vc.ln.f, vc.ln.gamma4pi, vc.ln.nujk};
        const LineScale s = line_scale(z, b, ln, cold);
        std::printf("{\"kind\": \"line_scale\", \"z\": \"%016" PRIx64 "\", \"b\": \"%016" PRIx64 "\", \"cold\": \"%016" PRIx64 "\", \"wrest_cm\": \"%016" PRIx64
                    "\", \"f\": \"%016" PRIx64 "\", \"gamma4pi\": \"%016" PRIx64 "\", \"nujk\": \"%016" PRIx64 "\", \"rdnu\": \"%016" PRIx64
                    "\", \"zp1\": \"%016" PRIx64 "\", \"A\": \"%016" PRIx64 "\", \"B\": \"%016" PRIx64 "\", \"a\": \"%016" PRIx64 "\", \"K\": \"%016" PRIx64
                    "\", \"record_kind\": %d}\n", bits(z), bits(b), bits(cold), bits(ln.wrest_cm), bits(ln.f), bits(ln.gamma4pi), bits(ln.nujk),
                    bits(s.rdnu), bits(s.zp1), bits(s.A), bits(s.B), bits(s.a), bits(s.K), (int)record_kind(s.zp1, s.a, s.K));
    }
}

static void half_widths() {
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const double velstep = 2.0;
    const int n_cap = 10, jax_half = 7;
    auto reach = [&](double n) { return (n - 0.5) / kKernelReach * velstep * kFwhmToSigma; };   // an R whose ceil(kKernelReach sigma) is n
    const double Rs[] = {1.0, velstep, std::nextafter(velstep, 3.0), reach(9.0), reach(10.0), reach(11.0), 1e300, inf, nan, -3.0};
    for (int jax = 0; jax < 2; ++jax)
        for (double R : Rs) {
            const LsfWidth w = lsf_half_width(R, velstep, jax, jax_half, n_cap);
            std::printf("{\"kind\": \"half_width\", \"jax\": %d, \"R\": \"%a\", \"velstep\": \"%a\", \"jax_half\": %d, \"n_cap\": %d, \"n\": %d, \"bad\": %d}\n",
                        jax, R, velstep, jax_half, n_cap, w.n, w.bad ? 1 : 0);
        }
}

int main() {
    layouts();
    counts();
    line_scales();
    half_widths();
    return 0;
}
