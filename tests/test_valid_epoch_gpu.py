"""GenerativePairValidStep / ValidEpoch (apr_amd/fcgf/lib/validation.py = GenerativePairTrainer._valid_epoch,
FCGF_APR/lib/complement_trainer.py:514-681) against the same quantities chained from the existing public functions, the
no-synchronisation property of the step, and the first train -> validate run on learned features (lib/learned.py)."""
import time

import numpy as np
import pytest
import torch

from apr_amd import MinkowskiEngine as ME
from apr_amd import ops, synth
from apr_amd.fcgf.lib import apg
from apr_amd.fcgf.lib.eval import evaluate_hit_ratio, find_corr
from apr_amd.fcgf.lib.learned import train_and_validate
from apr_amd.fcgf.lib.metrics import corr_dist
from apr_amd.fcgf.lib.validation import GenerativePairValidStep, ValidEpoch
from apr_amd.fcgf.model import load_model
from apr_amd.fcgf.util.transform_estimation import est_quad_linear_robust

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SUB, RATIO, VS, STRENGTH = 1500, 4, 0.3, 0.1
# iterations of the learned-features test.  Measured (DESIGN.md section 14 has the held-out hit ratio per budget and seed): of
# 50 / 100 / 200 / 400 only 400 raised it for all three seeds, so the test takes the next doubling
TRAIN_ITERATIONS = 800


def _pair(dev, seed):
    """tests/test_train_step_gpu.py's small pair with the validation keys pcd0 / pcd1 / T_gt."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=16, n_azimuth=600)
    out = {}
    rng = np.random.default_rng(seed)
    for tag, xyz in (("0", xyz0), ("1", xyz1)):
        key = torch.from_numpy(xyz).to(dev)
        m = ops.build_map(ops.voxelize(key, VS, 0), want_first=True)
        ops.finalize_maps([m])
        out[f"sinput{tag}_C"] = m.coords
        out[f"sinput{tag}_F"] = torch.ones((m.n, 1), device=dev)
        p = key[m.first.long()].contiguous()
        out[f"pcd{tag}"] = [p]
        jit = torch.from_numpy(rng.normal(0, 0.1, (2 * m.n, 3)).astype(np.float32)).to(dev)
        out[f"pcd_nghb{tag}"] = [(p.repeat(2, 1) + jit).contiguous()]      # a stand-in APG cloud
    out["T_gt"] = torch.from_numpy(T).float()
    out["len_batch"] = [[int(out["sinput0_C"].shape[0]), int(out["sinput1_C"].shape[0])]]
    return out


def _models(dev):
    torch.manual_seed(0)
    enc = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    gen = apg.GenerativeMLP_54(in_channel=32, out_points=RATIO, bn_momentum=0.05).to(dev)
    return enc, gen


def _chained(enc, gen, pairs, strict):
    """The reference's loop body on the public functions that existed before the fused entry, one host round trip each."""
    enc.eval()
    gen.eval()
    rows = []
    with torch.no_grad():
        for d in pairs:
            F = [enc(ME.SparseTensor(d[f"sinput{k}_F"], coordinates=d[f"sinput{k}_C"])).F for k in ("0", "1")]
            xyz0, xyz1, T_gt = d["pcd0"][0], d["pcd1"][0], d["T_gt"]
            c0, c1 = find_corr(xyz0, xyz1, F[0], F[1], subsample_size=SUB)
            T_est = est_quad_linear_robust(c0, c1)
            cd = float(corr_dist(T_est, T_gt, xyz0.cpu(), xyz1.cpu()))
            rte = float(np.linalg.norm((T_est[:3, 3] - T_gt[:3, 3]).numpy()))
            with np.errstate(invalid="ignore"):
                rre = float(np.arccos((np.trace((T_est[:3, :3].t() @ T_gt[:3, :3]).numpy()) - 1) / 2))
            hit = evaluate_hit_ratio(c0, c1, T_gt, thresh=0.1)
            Tg = T_gt.double().numpy()
            d64 = np.sqrt((((c0.double().cpu().numpy() @ Tg[:3, :3].T + Tg[:3, 3]) - c1.double().cpu().numpy()) ** 2).sum(1) + 1e-6)
            reg = cham = 0
            for k in (0, 1):
                g = gen(F[k]) * VS
                reg = reg + apg.npr_regulariser(g, 'L2', 0.1)
                pts = apg.npr_points(g, d[f"sinput{k}_C"][:, 1:], VS, RATIO)
                cham = cham + apg.chamfer_distance(pts, d["pcd_nghb0" if strict else f"pcd_nghb{k}"][0])
            rows.append(dict(cd=cd, rte=rte, rre=rre, hit=hit, n=len(c0), T=T_est.numpy(), cham=float(cham / 2), reg=float(reg / 2),
                             border=int((np.abs(d64 - 0.1) <= 1e-5).sum()), xmax=float(xyz0.abs().max())))
    return rows


def test_valid_epoch_matches_the_chain_of_public_functions(dev):
    pairs = [_pair(dev, 3), _pair(dev, 5)]
    assert all(p["sinput0_C"].shape[0] > SUB for p in pairs)          # find_corr's subsample branch is the one taken
    enc, gen = _models(dev)
    enc.train()
    gen.eval()
    results = {}
    for strict in (True, False):
        step = GenerativePairValidStep(enc, gen, voxel_size=VS, point_generation_ratio=RATIO, regularization_strength=STRENGTH,
                                       subsample_size=SUB, strict_reference=strict)
        np.random.seed(11)
        out, rec = ValidEpoch(step, pairs)()
        assert enc.training and not gen.training                      # left in the mode they were in
        np.random.seed(11)
        ref = _chained(enc, gen, pairs, strict)
        enc.train()
        results[strict] = rec
        for r, w in zip(rec, ref):
            assert r[ops.VALID_N_CORR] == w["n"] == SUB
            assert r[ops.VALID_T_EST:ops.VALID_T_EST + 16].tobytes() == w["T"].astype(np.float32).tobytes()
            assert abs(int(r[ops.VALID_N_HIT]) - round(w["hit"] * w["n"])) <= w["border"]
            bound = 16 * EPS * w["xmax"]
            print(f"corr_dist {r[0]} / {w['cd']}  rte {r[1]} / {w['rte']}  rre {r[2]} / {w['rre']}  "
                  f"chamfer {r[21]!r} / {w['cham']!r}  reg {r[22]!r} / {w['reg']!r}")
            assert abs(float(r[ops.VALID_CORR_DIST]) - w["cd"]) <= bound and abs(float(r[ops.VALID_RTE]) - w["rte"]) <= bound
            if np.isnan(w["rre"]) or np.isnan(r[ops.VALID_RRE]):
                # float32 trace on the host against the exact one in the kernel: at the edge of the domain either may be NaN
                assert np.isnan(r[ops.VALID_RRE]) or float(r[ops.VALID_RRE]) < 1e-3
            else:
                assert abs(float(r[ops.VALID_RRE]) - w["rre"]) <= 8 * EPS / max(np.sin(w["rre"]), 1e-3) + 2 * EPS * w["rre"]
            # the same kernels on the same inputs: measured bit-equal, so equality is what is asserted
            assert float(r[ops.VALID_CHAMFER]) == w["cham"] and float(r[ops.VALID_REG]) == w["reg"]
        # the seven keys, with the reference's arithmetic on the chained values
        ok = [w["rre"] for w in ref if not np.isnan(w["rre"])]
        want = {"loss": np.mean([v for w in ref for v in (w["cd"], np.float32(w["cham"]) + np.float32(w["reg"]) * np.float32(STRENGTH))]),
                "rre": np.mean(ok) if ok else 0.0, "rte": np.mean([w["rte"] for w in ref]),
                "feat_match_ratio": np.mean([w["hit"] > 0.05 for w in ref]), "hit_ratio": np.mean([w["hit"] for w in ref]),
                "chamfer_distance": np.mean([w["cham"] for w in ref]), "regularize_loss": np.mean([w["reg"] for w in ref])}
        assert set(out) == set(want)
        for k in want:
            assert abs(out[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (k, out[k], want[k])
    a, b = results[True], results[False]
    same = [c for c in range(ops.VALID_RECORD_FLOATS) if c != ops.VALID_CHAMFER]
    assert a[:, same].tobytes() == b[:, same].tobytes()               # strict_reference changes frame 1's Chamfer target only
    assert (a[:, ops.VALID_CHAMFER] != b[:, ops.VALID_CHAMFER]).all()


def test_the_step_enqueues_without_a_host_synchronisation(dev):
    pair = _pair(dev, 3)
    enc, gen = _models(dev)
    step = GenerativePairValidStep(enc, gen, voxel_size=VS, point_generation_ratio=RATIO, subsample_size=SUB)
    rec = torch.zeros((3, ops.VALID_RECORD_FLOATS), device=dev)
    prepared = step.prepare(pair)                  # the coordinate pyramids: the one part that fetches sizes, once per pair
    np.random.seed(1)
    step(prepared, rec, 0)                         # first call: weight packs, pinned staging buffer
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            np.random.seed(1)
            step(prepared, rec, 1)
            np.random.seed(1)
            step(prepared, rec, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    r = rec.cpu().numpy()
    assert r[0].tobytes() == r[1].tobytes() == r[2].tobytes() and r[0, ops.VALID_N_CORR] == SUB


def test_training_raises_the_held_out_hit_ratio_and_repeats_bit_for_bit(dev):
    """Learned features, reduced budget: ResUNetBN2C-32 on 16 x 600-ray pairs, 4 training and 3 held-out pairs."""
    t0 = time.perf_counter()
    kw = dict(n_train=4, n_val=3, iterations=TRAIN_ITERATIONS, model="ResUNetBN2C", n_out=32, n_beams=16, n_azimuth=600,
              seed=0, k=2, lr=0.05, num_pos=256, num_hn=128, register=False)
    a = train_and_validate(dev, **kw)
    b = train_and_validate(dev, **kw)
    print(f"{time.perf_counter() - t0:.1f} s; before {a['valid_before']}; after {a['valid_after']}; "
          f"loss {a['losses'][0]:.4f} -> {a['losses'][-1]:.4f}")
    assert a["losses"] == b["losses"] and len(a["losses"]) == TRAIN_ITERATIONS
    assert a["valid_before"] == b["valid_before"] and a["valid_after"] == b["valid_after"]
    for key in ("records_before", "records_after"):
        assert a[key].tobytes() == b[key].tobytes()
        assert np.isfinite(a[key]).all()
    assert np.isfinite(a["losses"]).all()
    assert all(np.isfinite(v) for d in (a["valid_before"], a["valid_after"]) for v in d.values())
    assert a["valid_after"]["hit_ratio"] > a["valid_before"]["hit_ratio"]
