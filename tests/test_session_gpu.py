"""Random call sequences on one engine against the oracle (tests/session_cases.py has the contract, the cells, the generator and the
runner; tests/test_session_host.py shows that the generator covers what it claims and that the runner notices seeded defects).  One
test per committed (cell, seed): every observation equals the shadow's, and the session reached the state its cell is about.
A failure names cell, seed and step: ``python tests/session_replay.py CELL SEED`` replays it."""
import numpy as np
import pytest

from lp_mp_amd import engine as E

import session_cases as SC

pytestmark = pytest.mark.gpu

MB = 1 << 20


def _run(cell, seed, monkeypatch, pair=False):
    v = SC.variant(cell, seed)
    for k, x in v["env"].items():
        monkeypatch.setenv(k, x)
    engines, skip = [], {}
    reach = SC.Reach()
    try:
        if pair and cell in ("windows", "relabel_windows"):    # the first engine: plain launches throughout, the second one follows the session (chain launches)
            engines.append(E.Engine(0))
            engines[0].set_persistent_launches(False)
            skip = {0: {"set_persistent_launches"}}
        elif pair:                    # the first engine: no passes ahead of the caller, the publishing records without LDS
            monkeypatch.setenv("LPMP_PQ_LDS", "0")
            engines.append(E.Engine(0))
            monkeypatch.delenv("LPMP_PQ_LDS")
            skip = {0: {"set_speculation"}}
        engines.append(E.Engine(0))
        session = SC.steps(cell, seed)
        SC.run(engines, SC.Shadow(), session, observe=SC.observe_plan(cell, seed, session), cell=cell, seed=seed,
               borrowed=v["borrowed"], reach=reach, skip=skip)
        if not pair:
            # the batches and roll-backs the engine counts are those the speculation paragraph of the header predicts for these steps
            # (session_cases.SpecSim; the comparisons after the last step settle once more)
            _, sim = SC.spec_trace(cell, seed, session)
            sim.settle()
            print(cell, seed, "batches / rollbacks", reach.batches, reach.rollbacks, "predicted", sim.batches, sim.rollbacks)
            assert (reach.batches, reach.rollbacks) == (sim.batches, sim.rollbacks), (vars(reach), sim.batches, sim.rollbacks)
        return reach, v
    except E.EngineError as ex:
        if ex.code == SC.ERR_DEVICE:          # nothing more is started on a device that reported an error
            pytest.exit("device error in session %s seed %s: %s" % (cell, seed, ex), returncode=3)
        raise
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("cell,seed", SC.sessions())
def test_session(cell, seed, monkeypatch):
    """(the windows cell, 113 factors: with duals bit-identical the bounds differed from the oracle's by at most 6.1e-15 relative over
    its four sessions, Reach.lb_rel_max — the suite's LB_RTOL = 1e-9 holds for DIFF_SHIFT models, no constant of its own)"""
    reach, v = _run(cell, seed, monkeypatch)
    print(cell, seed, vars(reach))
    if cell == "joined32":
        assert reach.peer_minima > 0 and reach.batches > 0 and reach.rollbacks > 0, vars(reach)
        if "LPMP_CHAIN_CACHE_MB" in v["env"]:
            assert 0 < reach.cache_max <= MB and reach.evictions > 0, vars(reach)
    elif cell == "mixed4":
        assert v["prec"] in reach.precisions, vars(reach)
    elif cell == "rows":
        assert reach.rows
    elif cell == "deep":
        assert reach.deep_chain_passes > 0, vars(reach)
    elif cell == "diffpool":
        assert reach.banded and reach.full, vars(reach)
    elif cell == "windows":
        # windows moved, timed launches of the shifted kernel, both label counts (SC.run checked schedules_built around every
        # window_set_create — one more — and every move_windows — unmoved)
        assert reach.moves > 0 and reach.window_sets > 0 and reach.shift_launches > 0 and reach.models == {"shift24", "shift72"}, vars(reach)
    if cell.startswith("relabel"):
        # path and forest moves done, sets created (SC.run checked schedules_built around every create — one more — and every move —
        # unmoved —, and the duals behind every move: no byte changes), moves on labels that were all unset
        assert reach.path_moves > 0 and reach.forest_moves > 0 and reach.move_sets > 0 and reach.moves_on_unset > 0, vars(reach)
        assert reach.models == set(SC.CELLS[cell]["models"]), vars(reach)
    if cell == "relabel":
        assert v["prec"] in reach.precisions and reach.rows, vars(reach)
    elif cell == "relabel_windows":
        # both label counts (the wave form and the workgroup form of the move kernels), a path or forest move on a set that was made
        # before a move_windows
        assert reach.moves > 0 and reach.moves_behind_windows > 0, vars(reach)


@pytest.mark.parametrize("seed", SC.HOP_SEEDS)
def test_one_engine_moves_through_four_models(seed, monkeypatch):
    reach, _ = _run("hop", seed, monkeypatch)
    print("hop", seed, vars(reach))


@pytest.mark.parametrize("cell,seed", [("joined32", 0), ("mixed4", 2), ("windows", 1), ("relabel", 2), ("relabel_windows", 1)])
def test_two_engines_run_the_same_session(cell, seed, monkeypatch):
    """one engine without passes ahead and with LPMP_PQ_LDS=0, one with the defaults (windows: one engine with plain launches
    throughout, one that follows the session's set_persistent_launches): both equal the shadow, and each other bit for bit (bounds
    as tests/test_speculation_gpu.py lines 115-121 allow).  relabel: as joined32 and mixed4; relabel_windows: as windows"""
    reach, _ = _run(cell, seed, monkeypatch, pair=True)
    if cell == "joined32":
        assert reach.peer_minima > 0 and reach.batches > 0, vars(reach)
    if cell == "windows":
        assert reach.moves > 0 and reach.models == {"shift24", "shift72"}, vars(reach)
    if cell.startswith("relabel"):
        assert reach.path_moves > 0 and reach.forest_moves > 0 and reach.models == set(SC.CELLS[cell]["models"]), vars(reach)
