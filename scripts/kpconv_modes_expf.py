"""One-off measurement behind E_EXP of tests/kpconv_modes_oracle.py: the error of the device's expf as
the gaussian influence evaluates it, against float64, over 2^20 arguments spanning [0, 110] (the cases' range: in-ball
arguments below 6, the far support's above 100).

Every argument goes through the library itself: query i at the origin with ONE neighbour at (t_i, 0, 0), kernel point 0 at
the origin, one feature channel equal to 1 -- apr_kpconv_weighted_mode(gaussian, sum) then returns wf[i, 0] = expf(-fl(t_i^2)
/ den) with den the kernel's float32 2 sigma^2 + 1e-9.  The float32 argument is restated here bit for bit (one product, one
correctly rounded division), so what is left is expf's own error.  Unit: eps32 |w| (an upper bound of w's ulp), results
under the smallest normal float32 excluded (the oracle covers them with an absolute term).

    python scripts/kpconv_modes_expf.py        ->  one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from apr_amd.predator import kp_ops  # noqa: E402


def main():
    n, extent = 1 << 20, np.float32(1.2)
    rng = np.random.default_rng(0)
    sg = 0.3 * float(extent)
    den = np.float32(2.0 * sg * sg + 1e-9)
    a = np.concatenate([rng.uniform(0.0, 110.0, n // 2), np.exp(rng.uniform(np.log(1e-6), np.log(110.0), n // 2))])
    t = np.sqrt(a * float(den)).astype(np.float32)
    arg = ((t * t).astype(np.float32) / den).astype(np.float32)      # what the kernel divides and negates, bit for bit
    dev = torch.device("cuda:0")
    s = np.zeros((n, 3), np.float32)
    s[:, 0] = t
    kp = np.full((15, 3), 100.0, np.float32)
    kp[0] = 0.0
    wf = kp_ops.kpconv_weighted(torch.zeros((n, 3), device=dev), torch.from_numpy(s).to(dev),
                                torch.arange(n, dtype=torch.int32, device=dev).view(n, 1),
                                torch.ones((n, 1), device=dev), torch.from_numpy(kp).to(dev), float(extent), mode=(2, 0))
    w = wf[:, 0].double().cpu().numpy()
    ref = np.exp(-arg.astype(np.float64))
    normal = ref >= 2.0 ** -126
    err = np.abs(w - ref)[normal] / (float(np.finfo(np.float32).eps) * ref[normal])
    sub = ~normal
    print(json.dumps(dict(arguments=int(n), normal=int(normal.sum()), worst_eps32=float(err.max()), mean_eps32=float(err.mean()),
                          at_argument=float(arg[normal][err.argmax()]), subnormal=int(sub.sum()),
                          subnormal_returned_nonzero=int((w[sub] != 0).sum()),
                          subnormal_worst_abs=float(np.abs(w - ref)[sub].max()) if sub.any() else 0.0)))


if __name__ == "__main__":
    main()
