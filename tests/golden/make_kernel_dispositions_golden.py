"""Generates tests/golden/kernel_dispositions.npz with the REFERENCE itself (build container only; needs /root/reference;
never run on a GPU machine):
    python tests/golden/make_kernel_dispositions_golden.py

Imports /root/reference/Predator_APR/kernels/kernel_points.py as it is, with the working directory in a temp dir (the
reference writes its dispositions under ./kernels/dispositions).  For (K, fixed) in (4, 'verticals'), (7, 'center'),
(13, 'none'), (16, 'center'), each under np.random.seed(3):
  raw/<K>_<fixed>   float64 [K, 3]: candidate 0 of kernel_point_optimization_debug(1.0, K, num_kernels=100, fixed=fixed)
  lk/<K>_<fixed>    float32 [K, 3]: load_kernels(1.5, K, 3, fixed) called on a FRESH directory (the disposition is made,
                    candidate argmin(grad_norms[-1]) taken, rotated, jittered, scaled)
  stop/<K>_<fixed>  int: the number of non-zero rows of saved_gradient_norms (the iteration the descent stopped at, + 1)
Only arrays are stored.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Predator_APR"
CASES = [(4, "verticals"), (7, "center"), (13, "none"), (16, "center")]


def main():
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    out = {}
    try:
        os.chdir(tempfile.mkdtemp())
        from kernels import kernel_points as ref
        for K, fixed in CASES:
            np.random.seed(3)
            pts, norms = ref.kernel_point_optimization_debug(1.0, K, num_kernels=100, dimension=3, fixed=fixed, verbose=0)
            out[f"raw/{K}_{fixed}"] = np.asarray(pts[0], np.float64)
            out[f"stop/{K}_{fixed}"] = np.int64((norms.max(1) > 0).sum())
            os.chdir(tempfile.mkdtemp())      # a fresh directory: load_kernels makes the disposition itself
            np.random.seed(3)
            lk = ref.load_kernels(1.5, K, 3, fixed)
            assert lk.dtype == np.float32 and lk.shape == (K, 3)
            out[f"lk/{K}_{fixed}"] = lk
            print(K, fixed, "stopped after", int(out[f"stop/{K}_{fixed}"]), "iterations")
    finally:
        os.chdir(cwd)
        sys.path.remove(REF)
    np.savez(os.path.join(HERE, "kernel_dispositions.npz"), **out)


if __name__ == "__main__":
    main()
