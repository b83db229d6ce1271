"""replay one session of tests/test_session_gpu.py and print the first diverging step.
python tests/session_replay.py CELL SEED [--upto K] [--observe-all] [--fresh-at K]
  --upto K       only the first K steps (a prefix of a session is the session of that length)
  --observe-all  download and compare the duals after every step: settles every speculative batch, so it narrows down and does not
                 reproduce
  --fresh-at K   at step K a new engine takes over with the shadow's model and duals (schedules, read-outs and the live window, path
                 and forest sets are made again from the shadow's lists; the labels are uploaded where the model takes
                 lpmp_upload_primal): a divergence that goes away was stale state in the old engine, one that stays is a wrong kernel
One engine, one process; ends at the first mismatch.  For a finding of the tests, not for running something again and again."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import session_cases as SC
from lp_mp_amd import engine as E

ap = argparse.ArgumentParser()
ap.add_argument("cell"); ap.add_argument("seed", type=int)
ap.add_argument("--upto", type=int); ap.add_argument("--observe-all", action="store_true"); ap.add_argument("--fresh-at", type=int)
args = ap.parse_args()
v = SC.variant(args.cell, args.seed)
os.environ.update(v["env"])                     # (read when an engine is created)
session = SC.steps(args.cell, args.seed, args.upto)
engines = [E.Engine(0)]
try:
    SC.run(engines, SC.Shadow(), session, observe=None if args.observe_all else SC.observe_plan(args.cell, args.seed, session), cell=args.cell,
           seed=args.seed, borrowed=v["borrowed"], fresh_at=args.fresh_at, fresh=lambda: E.Engine(0),
           log=lambda i, op, a: print("%4d %s%r" % (i, op, a), flush=True))
    print("no divergence in %d steps" % len(session))
except SC.Mismatch as ex:
    print("DIVERGED\n%s" % ex)
    sys.exit(1)
finally:
    for e in engines:
        e.close()
