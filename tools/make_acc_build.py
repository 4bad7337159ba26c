#!/usr/bin/env python3
"""Diagnostic builds of the library.  The product source carries NO instrumentation and no ablation switches: this script
patches a copy of it in a scratch directory (build/acc_src) and compiles that into build/abl/<name>.so, to be selected
with MCALF_HIP_LIB.

    python tools/make_acc_build.py                       # build/abl/stamps.so: phase timestamps per work item + per-wave
                                                         # s_memtime accumulators (fold / barrier / node pass / direct)
    python tools/make_acc_build.py --count-interp        # ... plus counters of interpolated / seen segments
    python tools/make_acc_build.py --name noloop --no-stamps --abl-noloop          # component loop removed
    python tools/make_acc_build.py --name setup_abl1 --no-stamps --abl-setup 1     # set-up without taps (2: without records, 3: neither)
    python tools/make_acc_build.py --name nointerp --no-stamps --no-far-interp     # every pixel evaluated directly
    python tools/make_acc_build.py [variant] --check-hooks                         # apply the variant's patches, compile nothing

    MCALF_HIP_LIB=build/abl/stamps.so python tools/stamp_report.py B 1024
    MCALF_HIP_LIB=build/abl/stamps.so python tools/timeline_report.py C 4096

Every patch names the exact source text it hooks on and fails loudly when that text has changed; most hooks are the call
of a phase in fused_items (csrc/fused_item.h), patched before or behind it.  tests/test_tool_hooks.py runs --check-hooks
for every variant above, so a kernel edit that moves a hook fails the CPU suite."""
import argparse
import os
import shutil
import sys
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(root, "mc-alf_amd", "csrc")

ap = argparse.ArgumentParser()
ap.add_argument("--name", default="stamps")
ap.add_argument("--no-stamps", action="store_true")
ap.add_argument("--count-interp", action="store_true")
ap.add_argument("--abl-noloop", action="store_true")
ap.add_argument("--abl-setup", type=int, default=0, help="bit 0: no taps, bit 1: no records")
ap.add_argument("--no-far-interp", action="store_true")
ap.add_argument("--check-hooks", action="store_true", help="apply every patch of the variant to a throw-away copy and stop before compiling")
args = ap.parse_args()
if os.environ.get("MCALF_COUNT_INTERP"):
    args.count_interp = True

sys.path.insert(0, root)
import importlib  # noqa: E402
bld = importlib.import_module("mc-alf_amd.build")
work = tempfile.mkdtemp(prefix="mcalf_hooks_") if args.check_hooks else os.path.join(root, "build", "acc_src")
bld.copy_sources(work)
# everything the kernel object is built from, and the host files a patch may reach
FILES = bld.HASHED + ["ctx_plan.h", "host_abi.cpp", "host_launch.cpp", "host_wide.cpp", "host_pipeline.cpp"]
text = {f: open(os.path.join(work, f)).read() for f in FILES}
applied = 0


def rep(a, b, count=1):
    """Replace the hook `a` in whichever source file carries it (exactly `count` occurrences over all of them)."""
    global applied
    found = sum(text[f].count(a) for f in FILES)
    if found != count:
        sys.exit("make_acc_build: expected %d occurrence(s), found %d, of:\n%s" % (count, found, a))
    for f in FILES:
        text[f] = text[f].replace(a, b)
    applied += 1


def before(hook, code):
    rep(hook, code + hook)


def behind(hook, code):
    rep(hook, hook + code)


STAMP = ("do { if (threadIdx.x == 0 && w < 8192) g_stamps[w * 8 + (%d)] = %s; } while (0);")


def stamp(k):
    return "        " + STAMP % (k, "__builtin_amdgcn_s_memrealtime()" if k in (0, 7) else "__builtin_amdgcn_s_memtime()") + "\n"


# the calls of the phases in fused_items (fused_item.h), as they stand there
ITEM_LOOP = "    ItemLoads L;\n    request_item<kZeroPad, kSelfHalo, kInline, kStream>(a, w, tid0, L);\n\n    while (true) {\n"
TAKE_TICKET = "        take_ticket<F::kDeferTicket>(a, q, lds, tid, held, nu, nuNode);\n"
COMPONENT_LOOP = "        const int buf = component_loop<kLinesPerSync, F::kPreMask>(lds, tid, h, nu, tau, nuNode, farNode, segOk, wvU);\n"
CONVOLUTION = "        // ---- 3+4. convolution, continuum, likelihood terms ----"
MORE = "        const bool more = tNext < q.nItems;\n"
REDUCE = "        reduce_and_store<kInline, kStream>(a, lds, g, tid, reduces, h.bad, sum);\n"

if not args.no_stamps or args.count_interp:
    before("// acc += a * b and acc += a with the accumulator tied to its register",
           "__device__ unsigned long long g_stamps[8192 * 8];\n__device__ unsigned long long g_dbg[4];   // [0] interpolated segments, "
           "[1] segments seen, [2] interpolable\n__device__ unsigned long long g_acc[8192 * 32];\n#define CLK() __builtin_amdgcn_s_memtime()\n")
    before('// ---- kernel entry points for the host files (kernel_args.h) -------------------------------------------------------------',
           'extern "C" int mcalf_diag_read_stamps(unsigned long long* out, int n) {\n'
           '    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mcalf::g_stamps), (size_t)n * sizeof(unsigned long long));\n}\n'
           'extern "C" int mcalf_diag_read_dbg(unsigned long long* out) {\n'
           '    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mcalf::g_dbg), 4 * sizeof(unsigned long long));\n}\n'
           'extern "C" int mcalf_diag_read_acc(unsigned long long* out, int n) {\n'
           '    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mcalf::g_acc), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;\n}\n')

if args.count_interp:
    rep("        done = uniform64((mp | mn) & segOk);                 // (segOk carries bits 8j only, so `done` does too)\n",
        "        done = uniform64((mp | mn) & segOk);\n"
        "        if ((threadIdx.x & 63) == 0) { atomicAdd(&g_dbg[0], (unsigned long long)__popcll(done)); atomicAdd(&g_dbg[1], 8ULL); "
        "atomicAdd(&g_dbg[2], (unsigned long long)__popcll(segOk)); }\n")

if not args.no_stamps:
    # phase timestamps of every work item (thread 0; `w` = the item index in scope): 0 item begins, 1 set-up data in LDS,
    # 2 first barrier passed, 3 component loop done, 4 flux tile published, 5 terms done, 6 slot, 7 item ends
    rep(ITEM_LOOP, ITEM_LOOP.replace("\n    while (true) {\n", "    unsigned long long accs[4] = {0, 0, 0, 0};   // cycles of the fold, its barrier, the node pass, the direct pass\n"
                                     "\n    while (true) {\n") + stamp(0))
    behind(TAKE_TICKET, stamp(1))
    rep(COMPONENT_LOOP, stamp(2) + COMPONENT_LOOP.replace("wvU);\n", "wvU, accs);\n") + stamp(3) +
        "        if ((threadIdx.x & 63) == 0 && w < 8192) { unsigned long long* q4 = g_acc + w * 32 + 4 * (threadIdx.x >> 6); "
        "q4[0] = accs[0]; q4[1] = accs[1]; q4[2] = accs[2]; q4[3] = accs[3]; }\n        accs[0] = accs[1] = accs[2] = accs[3] = 0;\n")
    before(CONVOLUTION, stamp(4))
    behind(MORE, stamp(5))
    behind(REDUCE, "        do { if (threadIdx.x == 0 && w < 8192) g_stamps[w * 8 + 6] = blockIdx.x; } while (0);\n" + stamp(7))
    # per-wave cycle accumulators inside the component loop (component_loop, fold_group's call, eval_line)
    rep("                                              double nuNode, double& farNode, unsigned long long segOk, int wvU) {\n    int buf = 0;\n",
        "                                              double nuNode, double& farNode, unsigned long long segOk, int wvU, unsigned long long (&accs)[4]) {\n"
        "    int buf = 0;\n")
    rep("        double* tabs = lds.sTab + buf * (kLinesPerSync * kTabPad);\n        fold_group<kLinesPerSync>(lds, tabs, tid, cl0, ncl_run);\n"
        "        __syncthreads();\n        buf ^= 1;\n",
        "        const unsigned long long f0 = CLK();\n        double* tabs = lds.sTab + buf * (kLinesPerSync * kTabPad);\n"
        "        fold_group<kLinesPerSync>(lds, tabs, tid, cl0, ncl_run);\n        const unsigned long long f1 = CLK();\n        __syncthreads();\n"
        "        const unsigned long long f2 = CLK();\n        accs[0] += f1 - f0; accs[1] += f2 - f1;\n        buf ^= 1;\n")
    rep("eval_line<kPreMask>(tabs + l * kTabPad, nu, tau, nuNode, farNode, segOk, wvU);",
        "eval_line<kPreMask>(tabs + l * kTabPad, nu, tau, nuNode, farNode, segOk, wvU, accs[2], accs[3]);")
    rep("                                          double& farNode, unsigned long long segOk, int wv) {\n    const double A = tab[kLineLds + 1], B = tab[kLineLds + 2];",
        "                                          double& farNode, unsigned long long segOk, int wv, unsigned long long& accNode, unsigned long long& accDirect) {\n"
        "    const unsigned long long c0 = __builtin_amdgcn_s_memtime();\n    const double A = tab[kLineLds + 1], B = tab[kLineLds + 2];")
    before("    const unsigned doneLo = (unsigned)done, doneHi = (unsigned)(done >> 32);",
           "    const unsigned long long c1 = __builtin_amdgcn_s_memtime();\n    accNode += c1 - c0;\n")
    behind("        fmac_inplace(tau[j], t, P);\n    }\n    }\n", "    accDirect += __builtin_amdgcn_s_memtime() - c1;\n")

if args.abl_noloop:
    rep("    const int ncl_run = h.ncl;\n", "    const int ncl_run = 0;       // ABLATION: no component loop\n")
if args.abl_setup & 2:
    rep("    for (int slot0 = lane; slot0 < nSlotsRun; slot0 += 64) {\n", "    for (int slot0 = lane; slot0 < 0; slot0 += 64) {      // ABLATION: no records\n")
if args.abl_setup & 1:
    rep("    if (ntap8 <= 64) {                               // the usual case: one tap per lane, one exp\n",
        "    if (false) {                                     // ABLATION: no taps\n")
    rep("    } else {\n        double gsum = 0.0;\n", "    } else if (false) {\n        double gsum = 0.0;\n")
    rep("    const double bot = kZeroPad ? 1.0 : botOrdered;\n    const int ngen = ngenLane;\n", "    const double bot = 1.0;\n    const int ngen = 0;\n")
if args.no_far_interp:
    rep("constexpr bool kFarInterp = true;", "constexpr bool kFarInterp = false;")

if args.check_hooks:
    shutil.rmtree(work)
    print("make_acc_build: %d patches of variant '%s' apply" % (applied, args.name))
    sys.exit(0)
os.makedirs(os.path.join(root, "build", "abl"), exist_ok=True)
for f in FILES:
    open(os.path.join(work, f), "w").write(text[f])
out = os.path.join(root, "build", "abl", args.name + ".so")
bld.build_tree(work, out, stamp="instrumented:" + args.name)
print("built", out)
