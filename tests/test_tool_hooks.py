"""CPU: the diagnostic builds of tools/make_acc_build.py are patches of a copy of the kernel sources, each hooked on an exact
piece of source text -- the call of a phase of the fused kernel, mostly.  A kernel edit that moves such a text must not
leave the phase stamps, the interpolation counters and the ablation builds unbuildable without anybody noticing: every
variant applies all of its patches here (--check-hooks: nothing is compiled, nothing is written into the tree)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {
    "stamps": [],
    "count-interp": ["--count-interp"],
    "abl-noloop": ["--name", "noloop", "--no-stamps", "--abl-noloop"],
    "abl-setup-3": ["--name", "setup_abl3", "--no-stamps", "--abl-setup", "3"],
    "no-far-interp": ["--name", "nointerp", "--no-stamps", "--no-far-interp"],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_hook_of_the_diagnostic_builds_applies(variant):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_acc_build.py"), "--check-hooks"] + VARIANTS[variant],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "patches of variant" in res.stdout and " 0 patches" not in res.stdout, res.stdout


def test_a_moved_hook_is_reported(tmp_path):
    """The check is not vacuous: the same patches against a source whose hook text is gone fail, and name the text."""
    tool = open(os.path.join(ROOT, "tools", "make_acc_build.py")).read()
    hook = 'rep("constexpr bool kFarInterp = true;"'
    assert tool.count(hook) == 1
    broken = tmp_path / "tools" / "make_acc_build.py"
    broken.parent.mkdir()
    broken.write_text(tool.replace(hook, 'rep("constexpr bool kFarInterp = maybe;"'))
    os.symlink(os.path.join(ROOT, "mc-alf_amd"), tmp_path / "mc-alf_amd")
    os.symlink(os.path.join(ROOT, "include"), tmp_path / "include")
    res = subprocess.run([sys.executable, str(broken), "--check-hooks", "--no-stamps", "--no-far-interp"], capture_output=True, text=True)
    assert res.returncode != 0 and "kFarInterp = maybe" in res.stderr and "found 0" in res.stderr, res.stdout + res.stderr
