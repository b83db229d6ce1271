"""Generates tests/golden/ref_outputs.npz: what the reference programs of oracle/_ref (oracle/build_ref.py: the reference's CSR
container, union_find and two_smallest_elements, compiled from the reference sources) print for exactly the inputs
tests/test_oracle_ref.py hands them — so that those tests also run where the reference sources are absent.

    python tests/golden/make_ref_outputs.py        (needs the reference sources: oracle/build_ref.available())

Stored: `keys` (program name + ":" + sha256 of the input text) and `outputs` (the program's stdout), both as unicode arrays.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lp_mp_amd import model as M  # noqa: E402
from oracle import build_ref  # noqa: E402
from tests import test_oracle_ref as T  # noqa: E402


def main():
    assert build_ref.available(), "the reference sources are needed to record their programs' answers"
    rec = {}
    r = T.Ref(build_ref.build(), {}, record=rec)
    T.test_reference_container_is_a_row_major_csr(r)
    for mode in (M.REPAM_ANISOTROPIC, M.REPAM_DAMPED_UNIFORM):
        T.test_plan_weight_and_mask_arrays_have_the_layout_of_the_reference_container(r, mode)
    T.test_partitions_are_numbered_as_the_references_union_find_numbers_them(r)
    T.test_oracle_potts_message_equals_the_references_two_smallest_elements(r)
    # the inputs of the device test (test_device_two_min_equals_the_references_two_smallest_elements): no GPU needed to ask the
    # reference what it answers
    T._ref_two_smallest(r, [c[2] for c in T._potts_vectors(np.random.default_rng(22), 50, with_inf=False)])
    keys = sorted(rec)
    out = os.path.join(ROOT, "tests", "golden", "ref_outputs.npz")
    np.savez_compressed(out, keys=np.array(keys), outputs=np.array([rec[k] for k in keys]))
    print(f"{out}: {len(keys)} recorded runs")


if __name__ == "__main__":
    main()
