"""Writes the small synthetic DTU ground-truth files of this folder (ObsMask{N}_10.mat, Plane{N}.mat) for the command-line
test of rc_mvsnet_amd.dtu_eval (tests/test_gpu_dtu_eval.py).  The clouds themselves are not stored: ``scans()`` regenerates
them from rc_mvsnet_amd.synthetic.dtu_eval_scan.  ObsMask files are written zlib-compressed, Plane files uncompressed.
Needs scipy (only to write):  python tests/golden/dtu_eval/make_dtu_eval_fixtures.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SCANS = {1: 11, 4: 12}          # scan number -> seed


def scans():
    from rc_mvsnet_amd import synthetic
    return {k: synthetic.dtu_eval_scan(n_stl=3000, n_data=4000, extent=40.0, res=2.0, seed=seed) for k, seed in SCANS.items()}


def main():
    import numpy as np
    import scipy.io as sio
    for k, s in scans().items():
        sio.savemat(os.path.join(HERE, f"ObsMask{k}_10.mat"), {"ObsMask": s["obs_mask"], "BB": s["bb"], "Res": np.array([[s["res"]]])},
                    do_compression=True)
        sio.savemat(os.path.join(HERE, f"Plane{k}.mat"), {"P": s["plane"].reshape(4, 1)}, do_compression=False)


if __name__ == "__main__":
    main()
