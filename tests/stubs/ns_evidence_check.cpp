// Stand-alone driver of mc-alf_amd/csrc/ns_evidence.h for tests/test_nsrun_host.py: reads the dead logL of a run (raw doubles)
// and writes, as raw doubles, ln Z, H, the running ln Z and ln X after the rounds, then the normalised log weights.
//   ns_evidence_check <in.bin> <out.bin> <nlive> <K>
// Built by the test with -fsanitize=address,undefined; nothing of it is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ns_evidence.h"

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const long nlive = std::atol(argv[3]), K = std::atol(argv[4]);
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<double> logl;
    double v;
    while (std::fread(&v, sizeof v, 1, in) == 1) logl.push_back(v);
    std::fclose(in);
    const long ndead = (long)logl.size();
    if (nlive < 1 || K < 1 || ndead < nlive || (ndead - nlive) % K != 0) return 4;
    // the running value as mcalf_nested_advance keeps it, round by round
    mcalf::NsEvidence ev;
    for (long r = 0; r < (ndead - nlive) / K; ++r) ev.die(logl.data() + r * K, K, nlive, nullptr);
    const bool stop = ev.converged(logl[ndead - 1], 1e-3);
    std::vector<double> logw(logl.size());
    double logZ, H;
    mcalf::ns_finish(logl.data(), ndead, nlive, K, logw.data(), &logZ, &H);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 5;
    const double head[5] = {logZ, H, ev.logZ, ev.logX, stop ? 1.0 : 0.0};
    std::fwrite(head, sizeof(double), 5, out);
    std::fwrite(logw.data(), sizeof(double), logw.size(), out);
    std::fclose(out);
    return 0;
}
