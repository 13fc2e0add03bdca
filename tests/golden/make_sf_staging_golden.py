"""Records tests/golden/sf_staging_parent_sha256.json: run on the MI355X from a build of the commit whose bits are to be pinned
(the parent of the slab-list change):

    python tests/golden/make_sf_staging_golden.py [OUT.json]

It runs the case builder of tests/test_gpu_sf_staging.py.  Per size it takes the first pair of SEED_CANDIDATES with which that
build accepts at least 4 of the 5 matrices in every case of the size (both shapes, the three update modes), and records the seeds,
and per case the SHA-256 values of the lower triangles of G and Z, of rn and of the flags, and the flags themselves.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import torch  # noqa: E402

import test_gpu_sf_staging as T  # noqa: E402
from admm_net_amd import _lib  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    assert torch.cuda.is_available()
    _lib.load()
    dev = torch.device("cuda:0")
    seeds, cases = {}, {}
    for D in T.SIZES:
        for cand in T.SEED_CANDIDATES:
            got = {}
            for waves in T.shapes_of(D):
                for mode in T.P.MODES:
                    got[T.case_id(D, waves, mode)] = T.digest(T.run_case(dev, D, waves, mode, cand))
            worst = min(sum(f == 0 for f in g["flags"]) for g in got.values())
            print(f"D={D} seeds {cand}: fewest accepted {worst} of {T.B}", flush=True)
            if worst >= 4:
                seeds[str(D)] = list(cand)
                cases.update(got)
                break
        else:
            raise SystemExit(f"D={D}: no pair of SEED_CANDIDATES gives 4 of {T.B} accepted in every case")
    with open(out, "w") as fh:
        json.dump({"seeds": seeds, "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
