"""The ticket descriptors of the peer-minima launches, host side: tests/cpp/pq_desc_probe.cpp against
lp_mp_amd/csrc/order.cpp ticket_descriptors — band order, tiled order and skewed tiled order, explicit lists and the periodic
template, with and without wide consume blocks, and hand-made lists with 0, D and D + 1 dependencies; inline caps 0, 1 and D: every
descriptor field for field against tk_launch, tk_block, dep_off and dep."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_descriptors_against_the_ticket_tables(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    csrc = os.path.join(ROOT, "lp_mp_amd", "csrc")
    exe = str(tmp_path / "pq_desc_probe")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pq_desc_probe.cpp"), os.path.join(csrc, "order.cpp"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pq desc ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # 2 grids x 2 block sizes x 3 orders x (2 explicit + 1 periodic) tables, each at 5 caps, and the hand-made lists
    assert len(re.findall(r"dependencies per ticket", out.stdout)) == 2 * 2 * 3 * 3, out.stdout
    assert int(re.search(r"pq desc ok \((\d+) tickets\)", out.stdout).group(1)) > 10000, out.stdout
