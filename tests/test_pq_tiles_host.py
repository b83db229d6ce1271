"""The ticket order of the peer-minima launches, host side: tests/cpp/pq_tiles_probe.cpp against lp_mp_amd/csrc/order.cpp —
the skewed tiled order on 24 x 24, 40 x 24 and 33 x 47 grids of 32 labels with small forced geometries (tiles of 3 to 6 blocks, 1 and 3
sub-bands, lags 1 and 2, depths 2, 4, 8 and 16) at 4 to 33 passes, explicit tables and the periodic template: every (step, block)
once, every dependency before its ticket, the two orders of the published minima, one sub-band = tiled_order, no tiles = band_order."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skewed_tiled_order_on_the_emitted_tables(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    csrc = os.path.join(ROOT, "lp_mp_amd", "csrc")
    exe = str(tmp_path / "pq_tiles_probe")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pq_tiles_probe.cpp"), os.path.join(csrc, "order.cpp"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pq tiles ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # 3 grids x 3 tile sizes x 4 depths x 3 (sub-bands, lag) x 8 pass counts explicit; the periodic and the wide ones on top
    tables, pairs = (int(x) for x in re.search(r"\((\d+) tables, (\d+) ordered pairs\)", out.stdout).groups())
    assert tables >= 3 * 3 * 4 * 3 * 8 and pairs > 0, out.stdout
