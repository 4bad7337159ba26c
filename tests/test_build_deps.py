"""CPU: mc-alf_amd/build.py takes every object's dependencies from the sources' own #include "..." lines.  The compiler is the
oracle for that scanner (hipcc -MM, which also sees an include behind a macro or an #if), and what is stale is decided on a
copy of the sources with empty files as objects: nothing here compiles a kernel."""
import functools
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bld = importlib.import_module("mc-alf_amd.build")

HEADERS = sorted(f for f in os.listdir(bld.CSRC) if f.endswith(".h"))
ABI_HEADER = os.path.join("..", "..", "include", "mcalf_hip.h")     # as the files of csrc/ include it
T0 = 1_000_000_000                                                   # sources; objects are 100 s newer, a touched file 200 s
DEVICE_OBJECTS = {os.path.splitext(s)[0] + ".o" for s in bld.DEVICE_SOURCES}
HOST_OBJECTS = {os.path.splitext(s)[0] + ".o" for s in bld.HOST_SOURCES}


@functools.lru_cache(maxsize=None)
def compiler_deps(src):
    """The project's own files that the preprocessor reads for `src` under the flags it is built with, the source left out."""
    flags = bld.KERNEL_FLAGS if src in bld.DEVICE_SOURCES else bld.HOST_FLAGS
    res = subprocess.run([bld._hipcc()] + flags + ["-MM", src], cwd=bld.CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rule = " ".join(line.rstrip("\\") for line in res.stdout.splitlines() if not line.startswith("#"))   # (offload-bundle markers)
    target, _, deps = rule.partition(":")
    assert target.strip() == os.path.splitext(src)[0] + ".o", rule
    local = {os.path.normpath(d) for d in deps.split() if not os.path.isabs(d)}
    assert src in local
    return frozenset(local - {src})


def objects(sources):
    return {os.path.splitext(s)[0] + ".o" for s in sources}


@pytest.mark.parametrize("src", bld.SOURCES)
def test_scanned_dependencies_are_the_compilers(src):
    assert set(bld.closure(src)) == compiler_deps(src)
    assert compiler_deps(src) <= set(HEADERS) | {ABI_HEADER}


@pytest.fixture
def tree(tmp_path):
    """A copy of the sources, every object present (an empty file, with a stamp next to it) and newer than every source."""
    src, obj = str(tmp_path / "src"), str(tmp_path / "obj")
    bld.copy_sources(src)
    os.makedirs(obj)
    for dirpath, _, files in os.walk(src):
        for f in files:
            os.utime(os.path.join(dirpath, f), (T0, T0))
    for o in DEVICE_OBJECTS | HOST_OBJECTS:
        for name, text in ((o, ""), (o + ".hash", "stamp0")):
            with open(os.path.join(obj, name), "w") as fh:
                fh.write(text)
            os.utime(os.path.join(obj, name), (T0 + 100, T0 + 100))

    def stale(touched=None, stamp="stamp0"):
        if touched:
            os.utime(os.path.join(src, touched), (T0 + 200, T0 + 200))
        try:
            return objects(bld.stale_sources(src, obj, stamp))
        finally:
            if touched:
                os.utime(os.path.join(src, touched), (T0, T0))
    return stale


def test_a_newer_header_marks_exactly_the_objects_whose_compiler_list_names_it(tree):
    for h in HEADERS:
        assert tree(h) == objects(s for s in bld.SOURCES if h in compiler_deps(s)), h
    assert tree(os.path.join("include", "mcalf_hip.h")) == objects(s for s in bld.SOURCES if ABI_HEADER in compiler_deps(s))
    for s in bld.SOURCES:                                                # (and a newer source its own object)
        assert tree(s) == objects([s]), s


def test_nothing_touched_nothing_stale(tree):
    assert tree() == set()


def test_hmc_args_marks_the_two_files_that_include_it(tree):
    assert tree("hmc_args.h") == {"hmc_kernels.o", "host_hmc.o"}


def test_the_generated_tables_mark_every_object(tree):
    assert len(DEVICE_OBJECTS) == 11 and len(HOST_OBJECTS) == 20
    assert tree("voigt_tables.h") == DEVICE_OBJECTS | HOST_OBJECTS


def test_host_ctx_marks_every_host_object_and_no_device_object(tree):
    assert tree("host_ctx.h") == HOST_OBJECTS


def test_wave_row_marks_no_host_object(tree):
    got = tree("wave_row.h")
    assert got and got <= DEVICE_OBJECTS


def test_a_changed_stamp_marks_the_two_objects_that_carry_it(tree):
    assert tree(stamp="stamp1") == {"kernels.o", "host_abi.o"}


def test_a_missing_object_is_stale(tmp_path):
    src = str(tmp_path / "src")
    bld.copy_sources(src)
    assert bld.stale_sources(src, str(tmp_path / "obj"), "stamp0") == bld.SOURCES


def test_the_commands_of_a_tree_build_and_where_its_stamps_go(tmp_path, monkeypatch):
    """(The compiler is not run: the commands are recorded.)  One command per source in link order, then the link; the hash goes
    to the one file that reads it, and the two stamps are written next to their objects in the tree, wherever the caller stands."""
    src, cmds = str(tmp_path / "src"), []
    bld.copy_sources(src)
    monkeypatch.setattr(bld, "_run", lambda cmd, cwd=None: cmds.append((cmd, cwd)) or "")
    monkeypatch.chdir(tmp_path)
    assert bld.build_tree(src, "out.so", stamp="s1", defines=("X=1",), kernel_flags=("-DK",)) == "out.so"
    assert all(cwd == src for _, cwd in cmds) and len(cmds) == len(bld.SOURCES) + 1
    for (cmd, _), s in zip(cmds, bld.SOURCES):
        assert cmd[-5:] == ["-DX=1", "-c", s, "-o", os.path.splitext(s)[0] + ".o"]
        assert cmd[1:-5] == (bld.KERNEL_FLAGS + (["-DK"] if s == bld.KERNEL_SOURCE else []) if s in bld.DEVICE_SOURCES
                             else bld.HOST_FLAGS + (['-DMCALF_SRC_HASH="s1"'] if s == "host_abi.cpp" else []))
    assert cmds[-1][0][1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", "out.so"] + [os.path.splitext(s)[0] + ".o" for s in bld.SOURCES] + ["-ldl"]
    assert sorted(f for f in os.listdir(src) if f.endswith(".hash")) == ["host_abi.o.hash", "kernels.o.hash"]
    assert open(os.path.join(src, "kernels.o.hash")).read() == "s1" and os.listdir(str(tmp_path)) == ["src"]


def test_source_hash_refuses_a_header_that_hashed_does_not_name(tmp_path):
    src = str(tmp_path)
    bld.copy_sources(src)
    assert bld.source_hash(src) == bld.source_hash()
    with open(os.path.join(src, "new_stage.h"), "w") as fh:
        fh.write("#pragma once\n")
    with open(os.path.join(src, "kernels.hip"), "a") as fh:
        fh.write('#include "new_stage.h"\n')
    with pytest.raises(RuntimeError, match=r"new_stage\.h"):
        bld.source_hash(src)
