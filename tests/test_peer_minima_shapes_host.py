"""Peer minima of the joined passes on models beyond the colour-major grid, host side (tests/peer_minima_cases.py): every
case of the list is eligible through the real planner in both anisotropic modes; the list holds publishing and consuming records with
1-4 edges on side 0, on side 1 and on both; a table transposed on one flipped edge changes the oracle's duals (so the device tests on
these inputs can tell a reduction over the wrong side of a table from the right one); and the hazard proofs of
tests/cpp/peer_minima_probe.cpp and tests/cpp/wide_consume_probe.cpp hold on the same graphs (g++ alone, against order.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from lp_mp_amd import engine as E
from lp_mp_amd import model as M
from oracle.binding import Oracle

import peer_minima_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (M.REPAM_ANISOTROPIC, M.REPAM_ANISOTROPIC2)
# the windows of tests/test_peer_minima_shapes_gpu.py, and two of one band at lag 1
WINDOWS = ["8:2:4", "5:1:2", "16:2:3", "3:4:7", "1:1:2", "1:1:4"]


def test_the_list_is_what_it_says():
    cs = PC.cases()
    assert [c.name for c in cs] == PC.CASE_NAMES and {c.family for c in cs} == set(PC.FAMILIES)
    for c in cs:
        deg0, deg1 = np.bincount(c.edges[:, 0], minlength=c.n0), np.bincount(c.edges[:, 1], minlength=c.n1)
        assert max(deg0.max(), deg1.max()) <= PC.MAX_DEGREE, c.name
        m = c.model()
        E_ = c.edges.shape[0]
        assert m.n_factors == c.n0 + c.n1 + E_ and m.n_messages == 2 * E_, c.name
        T = c.tables()
        assert T.shape == (E_, PC.L, PC.L) and not any(np.array_equal(t, t.T) for t in T), c.name
        # edge e of the case is pairwise factor pairwise(e), between the unaries the case says, on the sides the case says
        pw = np.array([c.pairwise(e) for e in range(E_)])
        left_of = {(int(r), int(t)): int(l) for t, l, r in zip(m.m_type, m.m_left, m.m_right)}
        on0 = np.array([left_of[(f, 0)] for f in pw]); on1 = np.array([left_of[(f, 1)] for f in pw])
        assert len(left_of) == 2 * E_ and np.all(on0 != on1), c.name
        if c.family != "suggested":
            assert np.array_equal(np.where(c.flip, on1, on0), c.edges[:, 0]), c.name
            assert np.array_equal(np.where(c.flip, on0, on1), c.n0 + E_ + c.edges[:, 1]), c.name
            first = np.array([int(m.m_type[2 * e]) for e in range(E_)])
            assert np.array_equal(first == 1, c.side1_first), c.name
    named = {c.name: c for c in cs}
    assert named["thinned 13x11"].n0 > len(set(named["thinned 13x11"].edges[:, 0].tolist()))          # isolated unaries
    assert len(set(map(tuple, named["thinned 13x11"].edges.tolist()))) < len(named["thinned 13x11"].edges)   # parallel edges
    c = named["thinned 14x10"]
    assert len(set(c.edges[:, 0].tolist())) == c.n0 and len(set(c.edges[:, 1].tolist())) == c.n1      # every unary keeps an edge
    assert named["flipped 13x11"].flip.all() and 0 < named["random-flip 13x11"].flip.sum() < len(named["random-flip 13x11"].flip)
    assert any(c.side1_first.any() and not c.side1_first.all() for c in cs)


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_every_case_is_eligible_in_both_anisotropic_modes(name):
    p = E.Plan(PC.case(name).model())
    for mode in MODES:
        assert p.pass_rotates(mode), (name, mode)
        assert p.peer_minima(mode) == (True, ""), (name, mode)


def test_census_is_complete():
    """a condition on the inputs: over the list, publishing and consuming records with 1-4 edges all on side 0, all on side 1 and (from
    2 edges) on both; publishing records with 3 and 4 edges whose parked table (receive 0) and whose kept or twice-requested table
    (receive 1) is on side 0, and on side 1; waves of the wide consume form whose two records are not on the same sides"""
    total = {}
    for c in PC.cases():
        for k, v in PC.census(c).items():
            total[k] = total.get(k, 0) + v
    cells = PC.census_cells()
    assert len(cells) == 2 * 11 + 8 + 1 and ("publish", 1, "mixed") not in cells
    assert set(total) <= set(cells), set(total) - set(cells)
    assert [k for k in cells if total.get(k, 0) == 0] == []
    # the colour-major grid the other tests run fills none of the new cells
    n0, n1, e = PC.colour_major_graph(13, 11)
    old = PC.census(PC.Case("grid", "grid", n0, n1, e, np.zeros(len(e), bool), np.zeros(len(e), bool)))
    assert all(k[2] == "side 1" or k[-1] == 1 for k in old if k[0] == "publish") and all(k[2] == "side 0" for k in old if k[0] == "consume")
    assert ("consume", "wave", "sides differ") not in old


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_a_table_transposed_on_one_flipped_edge_shows_in_the_oracle(family):
    """the seeded defect: a kernel that reduced one table over the wrong side would compute exactly the model with that table
    transposed, so the oracle on that model must leave other duals after one pass than on the true one"""
    c = next(c for c in PC.cases() if c.family == family and c.edges.shape[0] > 20)
    flipped = np.flatnonzero(c.flip)
    assert flipped.size
    e = int(flipped[flipped.size // 2])
    m = c.model()
    T = c.tables()
    off = m.const_offsets()[c.pairwise(e)]
    assert np.array_equal(np.asarray(m.const_data[off: off + PC.L * PC.L]).reshape(PC.L, PC.L), T[e])
    T[e] = T[e].T.copy()
    mt = c.model(T)
    assert np.array_equal(np.asarray(mt.const_data[off: off + PC.L * PC.L]).reshape(PC.L, PC.L), T[e])
    for mode in MODES:
        o, ot = Oracle(m), Oracle(mt)
        for x in (o, ot):
            x.set_reparametrization(mode); x.ComputePass(1)
        d, dt = o.duals(), ot.duals()
        assert np.isfinite(d).all() and np.isfinite(dt).all()
        doff = m.dual_offsets()
        pw = c.pairwise(e)
        assert not np.array_equal(d[doff[pw]: doff[pw + 1]], dt[doff[pw]: doff[pw + 1]]), (c.name, e, mode)
        assert not np.array_equal(d, dt)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    csrc = os.path.join(ROOT, "lp_mp_amd", "csrc")
    out = {}
    d = tmp_path_factory.mktemp("probes")
    for name in ("peer_minima_probe", "wide_consume_probe"):
        out[name] = str(d / name)
        subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-o", out[name],
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(csrc, "order.cpp"), "-lpthread"])
    return out


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_hazard_proofs_on_the_same_graphs(name, probes, tmp_path):
    """eligibility, one ticket per block, dependencies backwards, the slot hazards, every factor's consecutive touches ordered; band
    order, tiled order and the periodic template; consume blocks of 4 and of 8 records"""
    path = str(tmp_path / "graph.txt")
    with open(path, "w") as f:
        f.write(PC.case(name).graph_text())
    for probe, ok in (("peer_minima_probe", "peer minima ok"), ("wide_consume_probe", "wide consume ok")):
        out = subprocess.run([probes[probe], path] + WINDOWS, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and ok in out.stdout and "FAILED" not in out.stdout, (probe, out.stdout[-3000:] + out.stderr[-2000:])


def test_the_probes_refuse_what_is_no_graph(probes, tmp_path):
    path = str(tmp_path / "graph.txt")
    with open(path, "w") as f:
        f.write("3 2\n0 0\n1 2\n")                       # b = 2 is no colour-1 unary of two
    for probe in probes.values():
        out = subprocess.run([probe, path, "8:2:4"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and " ok" not in out.stdout, out.stdout
        out = subprocess.run([probe, path], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, out.stdout
