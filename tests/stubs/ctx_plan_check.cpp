// tests/test_ctx_plan_host.py: what mcalf_create decides from a spec before it touches a device, planned on the CPU with
// mc-alf_amd/csrc/ctx_plan.h (the header host_abi.cpp: create_impl plans with) for a fixed list of specs.  One JSON record
// per line: the return code and the message, every CtxShape field, the segok words, and a 64-bit FNV-1a digest of the bytes of
// each table; doubles are printed as hex floats.  Built with -ffp-contract=off under AddressSanitizer and UBSan; the test
// compares the records with tests/golden/ctx_plan.json.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ctx_plan.h"

using namespace mcalf;

enum Defect { kNone, kNullSpec, kNullWl, kNullLines };

// A case, and the branch of the planner it is in the list for.  specres_max < 0: +infinity.
struct Case {
    const char* name;
    const char* why;
    long npix;
    const char* grid;        // log (2 km/s pixels) / linear / gap (a log grid that jumps by 30 pixels after pixel 299) / descending / shuffled
    double velstep;
    int nlines, ncompmax, nfill, freespecres;
    double specres_fixed, specres_max;
    int conv_mode, lps_env;
    Defect defect;
};

static const Case kCases[] = {
    // pixel counts and grid kinds (specres 8 km/s at 2 km/s per pixel: n_cap 6)
    {"log1", "one pixel: tile 8, no grid recognised", 1, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log7", "tile rounds up to 8", 7, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log8", "tile exactly 8", 8, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log9", "tile 16", 9, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log63", "a partial first segment, grid not recognised (n < 66): the tail repeats", 63, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log64", "exactly one segment", 64, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log65", "n = 65: below the grid recognition's n >= 66", 65, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log66", "n = 66: the grid recognition's first length", 66, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log128", "two whole segments, no virtual continuation", 128, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log130", "a last partial segment continued logarithmically", 130, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"log4000", "63 real segments", 4000, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"linear130", "a last partial segment continued linearly", 130, "linear", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"gap700", "a gap after pixel 299: its segment is not interpolable", 700, "gap", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"descending4000", "descending wavelengths: searchable", 4000, "descending", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"shuffled4000", "pixels out of order: seg_search 0", 4000, "shuffled", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    // tile edges
    {"tile4080", "the largest single tile at n_cap 6: (4096 - 12) & ~7", 4080, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"tile4081", "one pixel more: two balanced tiles of 2048, selfhalo 0", 4081, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"tiles3", "three tiles, the last one partial", 8192, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"tile4096", "no LSF: a single tile of all 4096 pixels, nu without virtual pixels", 4096, "log", 2.0, 2, 2, 1, 0, 1.0, 1.0, 0, -1, kNone},
    // LSF reach
    {"reach0", "rmax <= velstep: n_cap 0", 600, "log", 2.0, 2, 2, 1, 0, 2.0, 2.0, 0, -1, kNone},
    {"reach-fixed", "numpy mode, specres_fixed > specres_max provisions the halo", 600, "log", 2.0, 2, 2, 1, 0, 30.0, 8.0, 0, -1, kNone},
    {"reach-free", "freespecres: specres_fixed is ignored", 600, "log", 2.0, 2, 2, 1, 1, 30.0, 8.0, 0, -1, kNone},
    {"jax0", "JAX mode convolves even at rmax <= velstep", 600, "log", 2.0, 2, 2, 1, 0, 2.0, 2.0, 1, -1, kNone},
    {"jax32", "JAX mode, the largest half-width with 2 half + 1 <= npix", 65, "log", 1.0, 2, 2, 1, 0, 24.44208185053381, 24.44208185053381, 1, -1, kNone},
    {"jax33", "JAX mode, one more: refused", 65, "log", 1.0, 2, 2, 1, 0, 25.21802095689996, 25.21802095689996, 1, -1, kNone},
    {"jax-f32", "JAX mode: 6 + 6e-12 pixels is 6 after the float32 rounding", 65, "log", 1.0, 2, 2, 1, 0, 4.655634638201572, 4.655634638201572, 1, -1, kNone},
    {"numpy-f64", "numpy mode: the same reach is 7 in double", 65, "log", 1.0, 2, 2, 1, 0, 4.655634638201572, 4.655634638201572, 0, -1, kNone},
    // wide fall-back (one component-line: 8 ncl_cap + 2 n_cap <= 1950 doubles is what the LDS budget leaves at 4 lines per barrier)
    {"fit971", "the largest n_cap the LDS budget takes at ncl_cap 1", 5000, "log", 1.0, 1, 1, 0, 0, 753.0489027283512, 753.0489027283512, 0, -1, kNone},
    {"wide972", "one more: wide, n_cap 0, wide_n_cap kept", 5000, "log", 1.0, 1, 1, 0, 0, 753.8248418347174, 753.8248418347174, 0, -1, kNone},
    {"wide2016", "2 n_cap + 64 = 4096 would fit the tile's pixels, the budget does not: wide", 5000, "log", 1.0, 1, 1, 0, 0, 1563.9052688809807, 1563.9052688809807, 0, -1, kNone},
    {"wide2017", "2 n_cap + 64 > 4096: wide", 5000, "log", 1.0, 1, 1, 0, 0, 1564.6812079873466, 1564.6812079873466, 0, -1, kNone},
    {"wide-jax", "a wide JAX context keeps jax_half", 5000, "log", 1.0, 1, 1, 0, 0, 1563.9052688809807, 1563.9052688809807, 1, -1, kNone},
    {"wide-short", "an LSF wider than the whole spectrum (numpy: periodic)", 600, "log", 1.0, 1, 1, 0, 0, 1563.9052688809807, 1563.9052688809807, 0, -1, kNone},
    {"wide-6e7", "2 n_cap + 1 > 6e7: refused", 600, "log", 1.0e-3, 1, 1, 0, 0, 24054.11229735073, 24054.11229735073, 0, -1, kNone},
    // lines per barrier (n_cap 6: 5 lines fit while 8 ncl_cap + 12 <= 1110)
    {"lps-4lines", "ncl_cap 4: 5 saves no barrier", 600, "log", 2.0, 2, 2, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"lps-5lines", "ncl_cap 5: 5 saves a barrier and fits", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"lps-137", "ncl_cap 137: the last one at which 5 fits", 600, "log", 2.0, 1, 137, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"lps-138", "ncl_cap 138: 5 saves a barrier and does not fit", 600, "log", 2.0, 1, 138, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"lps-env4", "MCALF_LINES_PER_SYNC=4 over an automatic 5", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, 4, kNone},
    {"lps-env5", "MCALF_LINES_PER_SYNC=5 over an automatic 4: honoured", 600, "log", 2.0, 2, 2, 0, 0, 8.0, 8.0, 0, 5, kNone},
    {"lps-env5-refused", "MCALF_LINES_PER_SYNC=5 where 5 does not fit", 600, "log", 2.0, 1, 138, 0, 0, 8.0, 8.0, 0, 5, kNone},
    {"lps-env7", "MCALF_LINES_PER_SYNC outside {4, 5} is ignored", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, 7, kNone},
    {"ncl242", "8 ncl_cap + 2 n_cap = 1948: the last ncl_cap that fits with n_cap 6", 600, "log", 2.0, 1, 242, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"ncl243", "8 ncl_cap + 2 n_cap = 1956: the records push the LSF out of the tile (wide)", 600, "log", 2.0, 1, 243, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"ncl244", "8 ncl_cap = 1952: the fixed part alone exceeds the budget", 600, "log", 2.0, 1, 244, 0, 0, 8.0, 8.0, 0, -1, kNone},
    {"ncl243-reach0", "8 ncl_cap = 1944 with n_cap 0 fits", 600, "log", 2.0, 1, 243, 0, 0, 2.0, 2.0, 0, -1, kNone},
    // the refusals of check_spec, in its order
    {"bad-null-spec", "spec NULL", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNullSpec},
    {"bad-npix0", "npix 0", 0, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-null-wl", "wl NULL", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNullWl},
    {"bad-npix-large", "npix above 2^30 (the arrays are not read)", (1L << 30) + 1, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-nlines0", "nlines 0", 600, "log", 2.0, 0, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-null-lines", "lines NULL", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNullLines},
    {"bad-ncompmax", "ncompmax negative", 600, "log", 2.0, 2, -1, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-nfill", "nfill negative", 600, "log", 2.0, 2, 2, -1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-velstep", "velstep 0", 600, "log", 0.0, 2, 2, 1, 0, 8.0, 8.0, 0, -1, kNone},
    {"bad-conv-mode", "conv_mode 2", 600, "log", 2.0, 2, 2, 1, 0, 8.0, 8.0, 2, -1, kNone},
    {"bad-specres0", "specres_max 0", 600, "log", 2.0, 2, 2, 1, 1, 8.0, 0.0, 0, -1, kNone},
    {"bad-specres-inf", "specres_max infinite", 600, "log", 2.0, 2, 2, 1, 1, 8.0, -1.0, 0, -1, kNone},
};

// The LDS doubles of a workgroup in front of its tile region (ItemLds::tile: tables, records, taps, reduction slots, weights),
// at the case's lines per barrier and at the one-launch variant's 4: what the planner's own hand-written sum gave for
// every case that plans, recorded before the kernel's layout (kernel_args.h) took its place.
struct FixedLds {
    const char* name;
    long at_lps, at_4;
};
static const FixedLds kFixedLds[] = {
    {"log1", 4798, 3958},      {"log7", 4798, 3958},       {"log8", 4798, 3958},           {"log9", 4798, 3958},
    {"log63", 4798, 3958},     {"log64", 4798, 3958},      {"log65", 4798, 3958},          {"log66", 4798, 3958},
    {"log128", 4798, 3958},    {"log130", 4798, 3958},     {"log4000", 4798, 3958},        {"linear130", 4798, 3958},
    {"gap700", 4798, 3958},    {"descending4000", 4798, 3958}, {"shuffled4000", 4798, 3958}, {"tile4080", 4798, 3958},
    {"tile4081", 4798, 3958},  {"tiles3", 4798, 3958},     {"tile4096", 4786, 3946},       {"reach0", 4786, 3946},
    {"reach-fixed", 4826, 3986}, {"reach-free", 4798, 3958}, {"jax0", 4790, 3950},         {"jax32", 4850, 4010},
    {"jax-f32", 4798, 3958},   {"numpy-f64", 4800, 3960},  {"fit971", 5856, 5856},         {"wide972", 3914, 3914},
    {"wide2016", 3914, 3914},  {"wide2017", 3914, 3914},   {"wide-jax", 3914, 3914},       {"wide-short", 3914, 3914},
    {"lps-4lines", 3950, 3950}, {"lps-5lines", 4798, 3958}, {"lps-137", 5854, 5014},       {"lps-138", 5022, 5022},
    {"lps-env4", 3958, 3958},  {"lps-env5", 4790, 3950},   {"lps-env5-refused", 5022, 5022}, {"lps-env7", 4798, 3958},
    {"ncl242", 5854, 5854},    {"ncl243", 5850, 5850},     {"ncl243-reach0", 5850, 5850},
};

// 0 when the layout of a planned shape gives the recorded doubles and the shape's LDS sizes follow from it; a line on
// stderr and 1 otherwise (the test takes any as a failure).
static int check_layout(const char* name, const CtxShape& s) {
    const FixedLds* want = nullptr;
    for (const FixedLds& f : kFixedLds)
        if (std::strcmp(f.name, name) == 0) want = &f;
    if (!want) {
        std::fprintf(stderr, "%s: plans, and has no recorded LDS layout\n", name);
        return 1;
    }
    const ItemLds at_lps(s.lps, s.ncl_cap, s.n_cap), at_4(4, s.ncl_cap, s.n_cap);
    const size_t region = (size_t)tile_doubles(s.tile + 2 * s.n_cap);
    const bool ok = at_lps.tile == want->at_lps && at_4.tile == want->at_4 &&
                    s.lds_bytes == ((size_t)want->at_lps + region) * sizeof(double) &&
                    s.lds_bytes_inline == ((size_t)want->at_4 + region) * sizeof(double) &&
                    // the regions follow each other without a gap, in the kernel's order
                    at_lps.tab == 0 && at_lps.rec == 2L * s.lps * kTabPad && at_lps.taps - at_lps.rec == (long)s.ncl_cap * kRecStride &&
                    at_lps.red - at_lps.taps == 2L * s.n_cap + 8 && at_lps.wt - at_lps.red == kRedDoubles &&
                    at_lps.tile - at_lps.wt == 64 * VT_INODES;
    if (!ok)
        std::fprintf(stderr, "%s: LDS layout gives %ld / %ld doubles (lds_bytes %zu / %zu), recorded %ld / %ld\n", name, at_lps.tile, at_4.tile,
                     s.lds_bytes, s.lds_bytes_inline, want->at_lps, want->at_4);
    return ok ? 0 : 1;
}

static std::vector<double> make_wl(const char* grid, long n) {
    std::vector<double> wl(n);
    const std::string g = grid;
    for (long i = 0; i < n; ++i) {
        const long k = (g == "gap" && i >= 300) ? i + 30 : (g == "descending" ? -i : i);
        wl[i] = g == "linear" ? 6190.0 + 0.04 * (double)i : 6190.0 * std::exp((double)k * 2.0 / 2.99792458e5);
    }
    if (g == "shuffled") {                                 // Fisher-Yates with a 64-bit LCG
        uint64_t x = 20240611;
        for (long i = n - 1; i > 0; --i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(wl[i], wl[(long)((x >> 33) % (uint64_t)(i + 1))]);
        }
    }
    return wl;
}

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static std::string quoted(const std::string& s) {
    std::string q = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') q += '\\';
        q += c;
    }
    return q + "\"";
}

int main() {
    int bad = 0;
    for (const Case& c : kCases) {
        const long nalloc = c.npix > 0 && c.npix <= 100000 ? c.npix : 1;       // (a refused npix never has its arrays read)
        std::vector<double> wl = make_wl(c.grid, nalloc), flux(nalloc, 1.0), err(nalloc);
        for (long i = 0; i < nalloc; ++i) err[i] = 0.02 + 0.001 * (double)((i * 37) % 11);
        std::vector<mcalf_line> lines(c.nlines > 0 ? c.nlines : 1);
        for (size_t l = 0; l < lines.size(); ++l) lines[l] = mcalf_line{1548.204 + 2.577 * (double)l, 0.1899 / (double)(l + 1), 2.643e8};
        mcalf_spec sp = {};
        sp.npix = c.npix;
        sp.wl = c.defect == kNullWl ? nullptr : wl.data();
        sp.flux = flux.data();
        sp.err = err.data();
        sp.velstep = c.velstep;
        sp.nlines = c.nlines;
        sp.lines = c.defect == kNullLines ? nullptr : lines.data();
        sp.fill = mcalf_line{250.0, 0.1899, 2.643e8};
        sp.ncompmax = c.ncompmax;
        sp.nfill = c.nfill;
        sp.freespecres = c.freespecres;
        sp.freecont = 0;
        sp.specres_fixed = c.specres_fixed;
        sp.specres_max = c.specres_max < 0.0 ? INFINITY : c.specres_max;
        sp.contval_fixed = 1.0;
        sp.conv_mode = c.conv_mode;
        sp.device = -1;
        sp.asymmlike = 1;
        sp.asymm_n4 = 0.3;
        sp.asymm_n5 = 0.1;

        CtxShape s;
        CtxTables t;
        std::string msg;
        int rc = check_spec(c.defect == kNullSpec ? nullptr : &sp, &msg);
        const bool checked = rc == MCALF_OK;
        if (checked && (rc = plan_shape(sp, c.lps_env, &s, &msg)) == MCALF_OK) plan_tables(sp, &s, &t);
        if (rc == MCALF_OK) bad += check_layout(c.name, s);

        std::printf("{\"name\": %s, \"why\": %s, \"spec\": {\"npix\": %ld, \"grid\": \"%s\", \"velstep\": \"%a\", \"nlines\": %d, \"ncompmax\": %d, "
                    "\"nfill\": %d, \"freespecres\": %d, \"specres_fixed\": \"%a\", \"specres_max\": \"%a\", \"conv_mode\": %d, \"lps_env\": %d, "
                    "\"defect\": %d}, \"refused_by\": \"%s\", \"rc\": %d, \"msg\": %s",
                    quoted(c.name).c_str(), quoted(c.why).c_str(), c.npix, c.grid, c.velstep, c.nlines, c.ncompmax, c.nfill, c.freespecres,
                    c.specres_fixed, sp.specres_max, c.conv_mode, c.lps_env, (int)c.defect, rc == MCALF_OK ? "" : (checked ? "plan_shape" : "check_spec"),
                    rc, quoted(msg).c_str());
        if (rc == MCALF_OK) {
            std::printf(", \"shape\": {\"npix\": %ld, \"nlines\": %d, \"ncompmax\": %d, \"nfill\": %d, \"freespecres\": %d, \"freecont\": %d, \"conv_mode\": %d, "
                        "\"ndim\": %d, \"startind\": %d, \"endind\": %d, \"specres_fixed\": \"%a\", \"specres_max\": \"%a\", \"contval_fixed\": \"%a\", "
                        "\"velstep\": \"%a\", \"asymm\": %d, \"veto4\": \"%a\", \"veto5\": \"%a\", \"n_cap\": %d, \"tile\": %d, \"ntiles\": %d, \"ncl_cap\": %d, "
                        "\"jax_half\": %d, \"selfhalo\": %d, \"lps\": %d, \"lds_bytes\": %zu, \"lds_bytes_inline\": %zu, \"wide\": %d, \"wide_n_cap\": %d, "
                        "\"dnu_seg\": \"%a\", \"seg_nreal\": %d, \"seg_search\": %d}",
                        s.npix, s.nlines, s.ncompmax, s.nfill, s.freespecres, s.freecont, s.conv_mode, s.ndim, s.startind, s.endind, s.specres_fixed,
                        s.specres_max, s.contval_fixed, s.velstep, s.asymm, s.veto4, s.veto5, s.n_cap, s.tile, s.ntiles, s.ncl_cap, s.jax_half, s.selfhalo,
                        s.lps, s.lds_bytes, s.lds_bytes_inline, s.wide, s.wide_n_cap, s.dnu_seg, s.seg_nreal, s.seg_search);
            std::printf(", \"nu_len\": %zu, \"segok\": [", t.nu.size());
            for (size_t k = 0; k < t.segok.size(); ++k) std::printf("%s\"%016llx\"", k ? ", " : "", t.segok[k]);
            std::printf("], \"fnv\": {\"nu\": \"%016" PRIx64 "\", \"ispec2\": \"%016" PRIx64 "\", \"lgis\": \"%016" PRIx64 "\", \"lines\": \"%016" PRIx64 "\"}",
                        fnv1a(t.nu.data(), t.nu.size() * sizeof(double)), fnv1a(t.ispec2.data(), t.ispec2.size() * sizeof(double)),
                        fnv1a(t.lgis.data(), t.lgis.size() * sizeof(double)), fnv1a(t.lines.data(), t.lines.size() * sizeof(LineDev)));
        }
        std::printf("}\n");
    }
    return bad ? 1 : 0;
}
