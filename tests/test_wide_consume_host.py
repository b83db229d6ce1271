"""Wide consume blocks of the joined passes, host side: plan_rotation_chain with H / K / T blocks of 8 records beside W
blocks of 4, through joined_pass_tables — one ticket per block, dependencies backwards, the slot hazards of the published minima, and
every factor's consecutive touches ordered by ancestry; and the default parameter returns what it returned before
(tests/cpp/wide_consume_probe.cpp against lp_mp_amd/csrc/order.cpp, g++ alone)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_consume_blocks_on_the_emitted_tables(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    csrc = os.path.join(ROOT, "lp_mp_amd", "csrc")
    exe = str(tmp_path / "wide_consume_probe")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "wide_consume_probe.cpp"), os.path.join(csrc, "order.cpp"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "wide consume ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
