"""Peer minima of the joined passes, host side: which models may take the form (lpmp_plan_peer_minima on the planner's
real schedules; tests/cpp/peer_minima_probe.cpp on the rule itself), and the hazard proof — the slot of every pairwise factor, written
by the W record that receives-and-sends it and read by the K / T record at the other end, is ordered by the dependencies the joined
launch already has (band order, tiled order, periodic template; several pass counts)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from lp_mp_amd import synthetic as S

ANISO = M.REPAM_ANISOTROPIC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def star_model(L=32, leaves=5, arms=3, seed=5):
    """a bipartite graph in a 2-colour order: `arms` centres (colour 1) with `leaves` leaves (colour 0) each"""
    rng = np.random.default_rng(seed)
    b = M.ModelBuilder(2, S.mrf_mtypes())
    leaf = [[b.add_vector_factors(0, rng.uniform(0, 1, (1, L)))[0] for _ in range(leaves)] for _ in range(arms)]
    pw = [[b.add_dense_pairwise(1, rng.uniform(0, 1, (1, L, L)))[0] for _ in range(leaves)] for _ in range(arms)]
    centre = [b.add_vector_factors(0, rng.uniform(0, 1, (1, L)))[0] for _ in range(arms)]
    for a in range(arms):
        for i in range(leaves):
            b.add_messages(0, leaf[a][i], pw[a][i]); b.add_messages(1, centre[a], pw[a][i])
            b.add_relations(leaf[a][i], pw[a][i]); b.add_relations(pw[a][i], centre[a])
    return b.finish()


@pytest.mark.parametrize("H,W", [(2, 2), (1, 7), (3, 3), (13, 11), (14, 10), (40, 36)])
def test_colour_major_grids_of_32_labels_are_eligible(H, W):
    p = E.Plan(S.grid_model(H, W, 32, order="colour_major", seed=1))
    assert p.pass_rotates(ANISO)
    assert p.peer_minima(ANISO) == (True, "")
    for mode in (M.REPAM_UNIFORM, M.REPAM_DAMPED_UNIFORM):           # every message received and then sent: the same shape
        assert p.peer_minima(mode)[0] == p.pass_rotates(mode)


@pytest.mark.parametrize("name,model", [
    ("degree 5", lambda: star_model()),
    ("21 labels", lambda: S.grid_model(14, 10, 21, order="colour_major", seed=2)),
    ("16 labels", lambda: S.grid_model(14, 10, 16, order="colour_major", seed=2)),
    ("potts", lambda: S.grid_model(14, 10, 32, pairwise="potts", order="colour_major", seed=2)),
    ("row major", lambda: S.grid_model(6, 5, 32, order="row_major", seed=2)),
])
def test_models_that_stay_on_the_old_form(name, model):
    ok, why = E.Plan(model()).peer_minima(ANISO)
    assert not ok and why, (name, why)


def test_four_leaves_are_eligible_and_five_are_not():
    assert E.Plan(star_model(leaves=4)).peer_minima(ANISO) == (True, "")
    assert not E.Plan(star_model(leaves=5)).peer_minima(ANISO)[0]


def test_rule_and_slot_hazards_on_the_emitted_tables(tmp_path):
    """tests/cpp/peer_minima_probe.cpp against lp_mp_amd/csrc/order.cpp (host only, g++)"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    csrc = os.path.join(ROOT, "lp_mp_amd", "csrc")
    exe = str(tmp_path / "peer_minima_probe")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "peer_minima_probe.cpp"), os.path.join(csrc, "order.cpp"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "peer minima ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
