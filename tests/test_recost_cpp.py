"""LP_gpu<FMC>::upload_costs (lp_mp_amd/include/LP_gpu.hxx) through tests/cpp/test_recost_gpu.cpp, compiled with g++ against the C ABI
library as tests/test_cpp_dropin.py does: the host part here, the run on the GPU — where its bounds must be the Python mirror's."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "test_recost_gpu"


def _build(tmp_path):
    from lp_mp_amd import build as B
    B.build()
    exe = str(tmp_path / NAME)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "lp_mp_amd", "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", NAME + ".cpp"),
                           "-L", B.CSRC, "-llpmp_engine", "-Wl,-rpath," + B.CSRC])
    return exe


def test_cpp_program_compiles_and_host_part_passes(tmp_path):
    out = subprocess.check_output([_build(tmp_path), "--host-only"], text=True)
    assert "all tests passed" in out


def _python_mirror():
    """the same calls through lp_mp_amd/lp.py"""
    from lp_mp_amd import lp as LPM, model as M
    U = LPM.FactorContainer(LPM.UnarySimplexFactor, 0, True)
    P = LPM.FactorContainer(LPM.PairwiseSimplexFactor, 1)
    ML = LPM.MessageContainer(LPM.UnaryPairwiseMessage(0), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 0)
    MR = LPM.MessageContainer(LPM.UnaryPairwiseMessage(1), 0, 1, M.SCHED_LEFT, M.variableMessageNumber, 1, 1)
    lp = LPM.LP(LPM.FMC("SRMP", [U, P], [ML, MR]))
    u1, u2 = lp.add_factor(U, [0.0, 1.0]), lp.add_factor(U, [1.0, 0.0])
    p = lp.add_factor(P, 2, 2, [[0.0, 1.0], [1.0, 0.0]])
    lp.add_message(ML, u1, p); lp.add_message(MR, u2, p)
    lp.AddFactorRelation(u1, p); lp.AddFactorRelation(p, u2)
    lp.Begin(); lp.set_reparametrization("anisotropic")
    bounds = [lp.LowerBound()]
    for i in range(3):
        lp.ComputePass(i)
    bounds.append(lp.LowerBound())
    lp.set_factor_cost(u1, [0.7, 0.1]); lp.set_factor_cost(p, 2, 2, [[0.0, 0.3], [0.6, 0.0]])
    lp.upload_costs()
    bounds.append(lp.LowerBound())
    for i in range(3):
        lp.ComputePass(i)
    bounds.append(lp.LowerBound())
    lp.set_factor_cost(u2, [0.25, 0.5]); lp.set_factor_cost(p, 2, 2, [[0.0, 2.0], [2.0, 0.0]])
    lp.upload_costs(warm=True)
    bounds.append(lp.LowerBound())
    for i in range(2):
        lp.ComputePass(i)
    bounds.append(lp.LowerBound())
    return bounds, lp.duals()[2:4]


@pytest.mark.gpu
def test_cpp_upload_costs_equals_the_python_mirror(tmp_path):
    out = subprocess.check_output([_build(tmp_path)], text=True, timeout=300)
    print(out)
    assert "all tests passed" in out
    got = [float(x) for x in re.findall(r"^bound (\S+)$", out, re.M)]
    want, u2 = _python_mirror()
    print(want, u2)
    assert len(got) == 6 and got == want                       # exactly: the same calls reach the same engine
    assert got[1] == 1.0 and got[2] != got[1] and got[4] != got[3]
    assert [float(x) for x in re.search(r"^u2 (\S+) (\S+)$", out, re.M).groups()] == list(u2)
