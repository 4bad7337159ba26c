"""Build libmcalf_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

This file is the one description of the build.  The library is the device files of DEVICE_SOURCES -- the likelihood's fused
kernel first, then the kernels of the analysis passes, the fit and the samplers -- and the host side of the C ABI,
HOST_SOURCES, compiled as plain C++ against the HIP runtime API, linked in that order.  What an object depends on is not
written down anywhere: it is its source and every project header that source includes, directly or through another
(closure()).  Objects are kept under csrc/obj/ so that an edit recompiles only the files that include what was edited (the
fused kernel alone takes 22 s)."""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
KERNEL_SOURCE = "kernels.hip"
# what the DEVICE code of the likelihood is made of -- kernels.hip and every header it includes, directly or through another
# (the stages of the fused kernel are a header each: ONE translation unit) -- the kernel-source hash covers exactly these, in
# THIS order (the records under profiles/ carry the value: source_hash() checks the set, the order is data)
HASHED = ["kernels.hip", "kernel_args.h", "voigt_device.h", "voigt_tables.h", "wave_util.h", "sample_setup.h", "stream_handover.h",
          "line_eval.h", "fused_item.h", "wide_lsf.h"]
# what the library is made of, in link order
DEVICE_SOURCES = [KERNEL_SOURCE, "grad_kernels.hip", "eqw_kernels.hip", "kin_kernels.hip", "band_kernels.hip", "fit_kernels.hip",
                  "ns_kernels.hip", "ns_round_kernels.hip", "ens_kernels.hip", "hmc_kernels.hip", "prior_kernels.hip"]
# the device files whose kernels' resource usage a verbose build prints (all but the gradient's)
REPORTED = [s for s in DEVICE_SOURCES if s != "grad_kernels.hip"]
HOST_SOURCES = ["host_abi.cpp", "host_launch.cpp", "host_wide.cpp", "host_pipeline.cpp", "host_stream.cpp", "host_config.cpp", "host_multi.cpp",
                "host_staged.cpp", "host_grad.cpp", "host_fit.cpp", "host_ns.cpp", "host_nsrun.cpp", "host_ens.cpp", "host_hmc.cpp", "host_prior.cpp", "host_eqw.cpp", "host_kin.cpp", "host_band.cpp", "broker.cpp", "comm.cpp"]
SOURCES = DEVICE_SOURCES + HOST_SOURCES
TARGET = os.path.join(CSRC, "libmcalf_hip.so")
OBJDIR = os.path.join(CSRC, "obj")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
KERNEL_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]
HOST_FLAGS = ["-x", "c++", "-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE]
HASH_MACRO = "MCALF_SRC_HASH"
_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _hipcc() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _read(path: str) -> str:
    with open(path) as fh:
        return fh.read()


def closure(src: str, srcdir: str = CSRC):
    """The project's own headers that `src` includes ("..." includes only), directly or through another, as sorted paths
    relative to `srcdir` (the C ABI's header, under include/ at the top of the tree, counts).  An object depends on its source
    and these."""
    seen, todo = set(), [src]
    while todo:
        f = todo.pop()
        for inc in _INCLUDE.findall(_read(os.path.join(srcdir, f))):
            inc = os.path.normpath(os.path.join(os.path.dirname(f), inc))
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return sorted(seen)


def dependencies(src: str, srcdir: str = CSRC):
    """What the object of `src` is built from: the source, then its closure."""
    return [src] + closure(src, srcdir)


def source_hash(srcdir: str = CSRC) -> str:
    """sha256 over the kernel sources (HASHED: kernels.hip and the headers it is built from), 16 hex digits.  The
    library carries it (mcalf_version()), the PMC-derived files under profiles/ are stamped with it, and bench.py drops
    their figures when the two differ -- a kernel edit cannot ship stale utilisation numbers, and an edit of the host
    side of the C ABI (the .cpp files) does not change what the counters measured.  A header the fused kernel includes
    and HASHED does not name (or the reverse) is an error here, before anything is compiled."""
    reached = {KERNEL_SOURCE, *closure(KERNEL_SOURCE, srcdir)}
    if reached != set(HASHED):
        raise RuntimeError("HASHED is not what %s is built from: it misses %s and names %s that the kernel does not include"
                           % (KERNEL_SOURCE, sorted(reached - set(HASHED)) or "nothing", sorted(set(HASHED) - reached) or "nothing"))
    h = hashlib.sha256()
    for f in HASHED:
        with open(os.path.join(srcdir, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _object(src: str, objdir: str) -> str:
    return os.path.join(objdir, os.path.splitext(src)[0] + ".o")


def _reads_hash(deps, srcdir: str) -> bool:
    return any(HASH_MACRO in _read(os.path.join(srcdir, f)) for f in deps)


def _stamped(deps, srcdir: str) -> bool:
    """Whether an object with these dependencies depends on the hash itself: the fused kernel's (the hash is of what it is
    built from; the stamp next to the object says which) and every file that reads the macro."""
    return deps[0] == KERNEL_SOURCE or _reads_hash(deps, srcdir)


def stale_sources(srcdir: str, objdir: str, stamp: str, sources=SOURCES):
    """Those of `sources` (files of `srcdir`) whose object in `objdir` has to be compiled: it is missing, it is older than the
    source or a header of its closure, or it carries the hash and was built under another stamp (kept in <object>.hash).
    Nothing is compiled or written here."""
    stale = []
    for src in sources:
        obj, deps = _object(src, objdir), dependencies(src, srcdir)
        fresh = os.path.exists(obj) and all(os.path.getmtime(os.path.join(srcdir, d)) <= os.path.getmtime(obj) for d in deps)
        if fresh and _stamped(deps, srcdir):
            fresh = os.path.exists(obj + ".hash") and _read(obj + ".hash").strip() == stamp
        if not fresh:
            stale.append(src)
    return stale


def _run(cmd, cwd=CSRC) -> str:
    res = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed (%s):\n%s%s" % (" ".join(cmd), res.stdout, res.stderr[-4000:]))
    return res.stderr


def _compile(src: str, srcdir: str, obj: str, stamp: str, testing=False, report=False, defines=(), kernel_flags=()) -> str:
    """Compile one file of `srcdir` into `obj`, the ONE place a compile command is put together: a device file gets the kernel
    flags (the fused kernel `kernel_flags` on top; with `report` the resource-usage remarks, which are returned), a host file
    the host flags; a file gets the hash only if it reads it, and -DMCALF_TESTING where the caller builds the test variant."""
    deps = dependencies(src, srcdir)
    if src in DEVICE_SOURCES:
        cmd = KERNEL_FLAGS + (list(kernel_flags) if src == KERNEL_SOURCE else []) + (["-Rpass-analysis=kernel-resource-usage"] if report else [])
    else:
        cmd = HOST_FLAGS
    cmd = cmd + ([f'-D{HASH_MACRO}="{stamp}"'] if _reads_hash(deps, srcdir) else []) + (["-DMCALF_TESTING"] if testing else [])
    log = _run([_hipcc()] + cmd + [f"-D{d}" for d in defines] + ["-c", src, "-o", obj], cwd=srcdir)
    if _stamped(deps, srcdir):
        with open(os.path.join(srcdir, obj + ".hash"), "w") as fh:         # (`obj` may be relative to `srcdir`, as the command has it)
            fh.write(stamp)
    return log


def _link(objs, target: str, cwd: str) -> None:
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target] + objs + ["-ldl"], cwd=cwd)


def build(force: bool = False, verbose: bool = False, testing: bool = False, target: str | None = None) -> str:
    """Compile what is stale (stale_sources; with `force` everything) and link the library if anything is newer than it.

    testing=True builds the TEST variant (-DMCALF_TESTING: the failure-injection hooks MCALF_TEST_FAIL_PREFLIGHT and
    MCALF_TEST_XCD_MASK exist only there) into `target` -- never the in-tree product library; it shares the product's
    device objects, so only the host files are compiled for it (into csrc/obj_testing/)."""
    if testing and not target:
        raise ValueError("a testing build needs an explicit target outside the product path")
    target = target or TARGET
    hostdir = OBJDIR + ("_testing" if testing else "")
    os.makedirs(OBJDIR, exist_ok=True)
    os.makedirs(hostdir, exist_ok=True)
    stamp = source_hash()
    device = DEVICE_SOURCES if force and not testing else stale_sources(CSRC, OBJDIR, stamp, DEVICE_SOURCES)
    host = HOST_SOURCES if force else stale_sources(CSRC, hostdir, stamp, HOST_SOURCES)
    for src in device:
        log = _compile(src, CSRC, _object(src, OBJDIR), stamp, report=verbose and src in REPORTED)
        if verbose:
            print(log)
    for src in host:
        _compile(src, CSRC, _object(src, hostdir), stamp, testing=testing)
    objs = [_object(s, OBJDIR) for s in DEVICE_SOURCES] + [_object(s, hostdir) for s in HOST_SOURCES]
    if device or host or not os.path.exists(target) or any(os.path.getmtime(o) > os.path.getmtime(target) for o in objs):
        _link(objs, target, CSRC)
    return target


def build_tree(workdir: str, target: str, stamp: str = "patched-copy", defines=(), kernel_flags=(), report: bool = False) -> str:
    """Compile a COPY of the sources (tools/make_acc_build.py and friends patch one: the product source carries no
    instrumentation) into `target`; with `report` the resource usage of every device file's kernels is returned instead of the
    path (resource_table picks a family by a part of its kernels' names)."""
    log = ""
    for src in SOURCES:
        log += _compile(src, workdir, _object(src, ""), stamp, report=report, defines=defines, kernel_flags=kernel_flags)
    _link([_object(s, "") for s in SOURCES], target, workdir)
    return log if report else target


def copy_sources(workdir: str) -> None:
    """A copy of everything the library is built from, laid out so that the copies' includes resolve inside `workdir`."""
    shutil.copytree(os.path.join(CSRC, "..", "..", "include"), os.path.join(workdir, "include"), dirs_exist_ok=True)
    for f in os.listdir(CSRC):
        if f.endswith((".h", ".hip", ".cpp")):
            txt = _read(os.path.join(CSRC, f))
            with open(os.path.join(workdir, f), "w") as fh:         # (the C ABI's header is two levels up in the tree)
                fh.write(txt.replace('#include "../../include/', '#include "include/'))


def resource_table(log: str, only: str = "fused"):
    """(kernel, VGPRs, scratch bytes per lane, occupancy, SGPR spills, VGPR spills) from a -Rpass-analysis log."""
    rows = []
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                         r".*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", log, re.S):
        if only in m.group(1):
            rows.append((m.group(1),) + tuple(int(m.group(k)) for k in range(2, 7)))
    return rows


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--incremental"]:     # (what the Makefile runs: compile what is stale, no more)
        print(build())
    elif sys.argv[1:]:
        sys.exit("usage: build.py [--incremental]")
    else:
        print(build(force=True, verbose=True))
