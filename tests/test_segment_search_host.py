"""CPU: the set-up's segment-mask words by boundary search against the walk over all 64 segments, word for word.

The segment-mask functions of mc-alf_amd/csrc/kernel_args.h are plain C++ that the set-up kernel and the host compile from one source.
tests/stubs/segment_search_check.cpp includes that header, builds the end tables of logarithmic grids of 4000, 130, exactly 128, 4080
and 63 pixels, of a grid with a seam, of a descending grid and of one whose last partial segment repeats its last value, and
compares seg_word_search with seg_word_walk (which places its bits by the word layout's definition, not by the transpose the
search uses) over random records and the adversarial ones: thresholds exactly on a grid value of |u| and one ulp to either
side, uthr = 0 / inf / NaN, A < 0, = 0, = inf and tiny, B = inf and NaN, A = B = inf, random holes in the context's mask.
Compiled with -ffp-contract=off, so that fma() is the only fused operation, as on the device.  The bar is zero mismatches.
The program also holds the precondition function mcalf_create decides with to: ascending, descending, equal neighbouring
ends and a seam pass; a shuffled grid, exchanged segments, a NaN or zero end fail."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_gives_the_walks_words(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "segment_search_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "mc-alf_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "stubs", "segment_search_check.cpp")], check=True)
    res = subprocess.run([exe, "400000"], capture_output=True, text=True)
    print(res.stdout)
    assert "FAIL" not in res.stdout and res.returncode == 0, res.stdout[-4000:]
    m = re.search(r"records (\d+) mismatches (\d+)", res.stdout)
    assert m and int(m.group(1)) >= 2_000_000 and int(m.group(2)) == 0
    for grid in ("log4000", "log130", "log128", "log4080", "seam700", "descending4000", "tail-repeated130"):
        assert re.search(r"^%s: npix" % grid, res.stdout, re.M), grid
