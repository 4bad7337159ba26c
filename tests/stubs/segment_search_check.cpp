// tests/test_segment_search_host.py: the segment-mask words by boundary search against the walk over every segment, word for
// word, both from mc-alf_amd/csrc/kernel_args.h (the source the set-up kernel compiles), and the precondition function
// mcalf_create decides with; the grids' pixel frequencies are laid out by mcalf_create's own fill_nu (ctx_plan.h).  Built with -ffp-contract=off; prints one line per grid and "FAIL ..." lines, exits 1 on any.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ctx_plan.h"
#include "kernel_args.h"

using namespace mcalf;

static const double kInf =std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

struct Grid {
    const char* name;
    std::vector<double> nu;      // 4096 entries, laid out by mcalf_create's fill_nu for a single-tile context
    long npix;
    uint64_t ok;                 // interpolable segments (bit m = segment m)
};

// A logarithmic grid of 2 km/s pixels from 6190 A (`dir` < 0: descending wavelengths), which fill_nu continues virtually up to
// the next multiple of 64 pixels (from 66 pixels on: a shorter grid repeats its last value), nu = 0 beyond; with `seam` the
// wavelengths jump by 30 pixels after pixel 299.
static Grid make_grid(const char* name, long npix, int dir = 1, bool seam = false, bool repeat_tail = false) {
    Grid g{name, std::vector<double>(4096, 0.0), npix, 0};
    const long upto = (npix + 63) & ~63L;
    std::vector<double> wl(npix);
    for (long i = 0; i < npix; ++i) {
        const long k = (seam && i >= 300) ? i + 30 : i;
        wl[i] = 6190.0 * std::exp((double)(dir * k) * 2.0 / 2.99792458e5);
    }
    fill_nu(wl.data(), npix, (long)g.nu.size(), g.nu.data());
    for (long i = npix; repeat_tail && i < upto; ++i) g.nu[i] = g.nu[i - 1];      // a grid create does not recognise: the last value repeated
    for (int m = 0; m < 64; ++m) {
        bool ok = true;
        if (64L * m < upto) {
            const double d = g.nu[64 * m + 63] - g.nu[64 * m];
            for (int i = 1; i < 64 && ok; ++i) ok = (g.nu[64 * m + i] - g.nu[64 * m + i - 1]) * d > 0.0;
            if (seam && 64 * m <= 300 && 300 < 64 * m + 64) ok = false;
        }
        if (ok) g.ok |= 1ull << m;
    }
    return g;
}

static double ulp_step(double x, int n) {
    for (; n > 0; --n) x = std::nextafter(x, kInf);
    for (; n < 0; ++n) x = std::nextafter(x, -kInf);
    return x;
}

static long g_records = 0, g_bad = 0;

static void check(const Grid& g, const double* ends, int nreal, double A, double B, double t, uint64_t ok) {
    const uint64_t want = seg_word_walk(A, B, t, ends, ok), got = seg_word_search(A, B, t, ends, nreal, ok);
    ++g_records;
    if (want != got && ++g_bad <= 10)
        std::printf("FAIL %s A=%a B=%a t=%a ok=%016llx walk=%016llx search=%016llx\n", g.name, A, B, t, (unsigned long long)ok,
                    (unsigned long long)want, (unsigned long long)got);
}

static void run_grid(const Grid& g, long nrandom, std::mt19937_64& rng) {
    int nreal = 0;
    if (!seg_ends_searchable(g.nu.data(), g.npix, &nreal)) {
        std::printf("FAIL %s: the precondition rejects the grid\n", g.name);
        ++g_bad;
        return;
    }
    double ends[kSegEnds];
    for (int k = 0; k < kSegEnds; ++k) ends[k] = g.nu[seg_end_pixel(k)];
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double nuA = ends[0], nuB = ends[2 * nreal - 1], span = nuB - nuA;
    const long before = g_records;
    auto holes = [&]() { return (rng() & 3) ? g.ok : (g.ok & rng() & rng()) | (rng() & (rng() & 1 ? ~0ull : 0ull)); };
    for (long r = 0; r < nrandom; ++r) {
        // a line centred inside the spectrum, at an end, or up to three spans outside, Doppler width 0.05 .. 60 km/s
        const int where = (int)(rng() % 8);
        double nu0 = where < 4 ? nuA + U(rng) * span : where == 4 ? ends[rng() % (2 * nreal)] : nuA + (U(rng) * 7.0 - 3.0) * span;
        const double w = nu0 * (0.05 + 60.0 * U(rng) * U(rng)) / 2.99792458e5;
        double A = 1.0 / w, B = nu0 / w;
        double t = (rng() % 4 == 0) ? 0.0 : 6.0 + 2.0 * U(rng);
        const int adv = (int)(rng() % 24);
        if (adv < 6) {                                   // the threshold exactly on a grid value of |u|, and an ulp to either side
            const double u = std::fma(ends[rng() % kSegEnds], A, -B);
            t = ulp_step(std::fabs(u), (int)(rng() % 3) - 1);
        } else if (adv == 6) t = kInf;
        else if (adv == 7) t = kNaN;
        else if (adv == 8) t = 1e300;
        else if (adv == 9) { A = -A; if (rng() & 1) B = -B; }
        else if (adv == 10) A = (rng() & 1) ? 0.0 : -0.0;
        else if (adv == 11) A = (rng() & 1) ? kInf : -kInf;
        else if (adv == 12) { A = 1e-300 * U(rng); B = (rng() & 1) ? A * nu0 : U(rng) * 1e-290; }
        else if (adv == 13) B = (rng() & 1) ? kInf : -kInf;
        else if (adv == 14) B = kNaN;
        else if (adv == 15) { A = kInf; B = kInf; }
        else if (adv == 16) A = kNaN;
        else if (adv == 17) { A = 4.9e-324; B = 0.0; t = 0.0; }
        else if (adv == 18) { A = 1e300; B = (rng() & 1) ? 1e308 : nu0; }
        check(g, ends, nreal, A, B, t, holes());
    }
    std::printf("%s: npix %ld, %d real segments, %ld records\n", g.name, g.npix, nreal, g_records - before);
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 600000;
    std::mt19937_64 rng(20240611);
    run_grid(make_grid("log4000", 4000), n, rng);
    run_grid(make_grid("log130", 130), n, rng);
    run_grid(make_grid("log128", 128), n, rng);
    run_grid(make_grid("log4080", 4080), n, rng);
    run_grid(make_grid("log63", 63), n / 4, rng);
    run_grid(make_grid("seam700", 700, 1, true), n, rng);
    run_grid(make_grid("descending4000", 4000, -1), n, rng);
    run_grid(make_grid("tail-repeated130", 130, 1, false, true), n / 4, rng);        // equal neighbouring ends

    // the precondition itself
    auto expect = [&](const char* what, bool got, bool want) {
        if (got != want) { std::printf("FAIL precondition: %s gives %d\n", what, (int)got); ++g_bad; }
    };
    int nreal = 0;
    Grid g = make_grid("log4000", 4000);
    expect("ascending wavelengths", seg_ends_searchable(g.nu.data(), g.npix, &nreal), true);
    expect("nreal of 4000 pixels", nreal == 63, true);
    expect("descending wavelengths", seg_ends_searchable(make_grid("d", 4000, -1).nu.data(), 4000, nullptr), true);
    expect("equal neighbouring ends", seg_ends_searchable(make_grid("r", 130, 1, false, true).nu.data(), 130, nullptr), true);
    expect("a grid with a seam", seg_ends_searchable(make_grid("s", 700, 1, true).nu.data(), 700, nullptr), true);
    {
        Grid e = g;                                      // two neighbouring ends made equal inside the grid
        e.nu[seg_end_pixel(11)] = e.nu[seg_end_pixel(10)];
        expect("equal ends inside the grid", seg_ends_searchable(e.nu.data(), e.npix, nullptr), true);
    }
    {
        Grid s = g;                                      // the real pixels shuffled
        std::shuffle(s.nu.begin(), s.nu.begin() + 4000, rng);
        expect("a shuffled grid", seg_ends_searchable(s.nu.data(), s.npix, nullptr), false);
        Grid w = g;                                      // one segment out of place
        std::swap_ranges(w.nu.begin() + 64, w.nu.begin() + 128, w.nu.begin() + 640);
        expect("two segments exchanged", seg_ends_searchable(w.nu.data(), w.npix, nullptr), false);
        Grid z = g; z.nu[seg_end_pixel(7)] = kNaN;
        expect("a NaN end", seg_ends_searchable(z.nu.data(), z.npix, nullptr), false);
        Grid o = g; o.nu[seg_end_pixel(7)] = 0.0;
        expect("a zero end among the real ones", seg_ends_searchable(o.nu.data(), o.npix, nullptr), false);
        Grid v = g; v.nu[4095] = 1.0;
        expect("a virtual end that is not 0", seg_ends_searchable(v.nu.data(), v.npix, nullptr), false);
    }
    // the transpose against the layout's definition
    for (int m = 0; m < 64; ++m)
        if (seg_transpose(1ull << m) != 1ull << (8 * (m & 7) + (m >> 3))) { std::printf("FAIL transpose of bit %d\n", m); ++g_bad; }
    std::printf("records %ld mismatches %ld\n", g_records, g_bad);
    return g_bad ? 1 : 0;
}
