"""The launch-size switch without a GPU: hbx::pass_launch_small (csrc/hbx_internal.hpp), the one place
that picks between the small and the walking forms of the first pass and of k_col2, against its Python
restatement tests/_launch_size.py -- the rule tests/test_gpu_launch_size.py chooses its job counts by."""
import os
import subprocess

import pytest

from tests import _launch_size as L
from tests.conftest import ROOT


def test_python_rule_at_the_documented_crossings():
    """DESIGN.md's table: the job counts per launch at which the walking forms start."""
    assert L.first_walking(1024, 8) == 16
    assert L.first_walking(1024, 2) == 64 and L.first_walking(1024, 8, pair=True) == 64
    assert L.first_walking(256, 8) == 64
    assert L.first_walking(256, 2) == 256 and L.first_walking(256, 8, pair=True) == 256
    # a pair is a pair whatever the group's plane count
    assert {L.first_walking(1024, p, pair=True) for p in L.TABLE_P} == {64}
    assert not L.walking(1024, 8, 15) and L.walking(1024, 8, 16) and L.walking(1024, 8, 17)
    assert L.first_walking(64, 8) == 1                     # N = 64: never small
    with pytest.raises(ValueError):
        L.walking(896, 8, 1)
    assert L.launches(18, 15) == [15, 3] and L.launches(16, 16) == [16] and L.launches(0, 4) == []


def test_host_table_equals_the_python_rule(tmp_path):
    """tests/c/launch_size_table.hip, a stand-alone host program (no GPU, no library), prints the first
    walking job count of every (R, P, pair); the Python rule gives the same table line for line."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "binary-hologram-reinforcement-learning_amd", "csrc")
    exe = str(tmp_path / "launch_size_table")
    subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "launch_size_table.hip"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(L.TABLE_R) * len(L.TABLE_P) * 2
    assert got == L.table(), "\n".join(f"{g!r} != {w!r}" for g, w in zip(got, L.table()) if g != w)
