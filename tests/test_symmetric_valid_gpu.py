"""SymmetricPairValidStep (apr_amd/fcgf/lib/validation.py = the symmetric branch of GenerativePairTrainer._valid_epoch,
FCGF_APR/lib/complement_trainer.py:575-581, :590-591, :622-623) against the float64 oracle chain in eval mode -- oracle
encoder, oracle ResUNetFatBN(128, 12) on its tensor, apr_step_oracle's regulariser / chamfer -- and a reduced
train_and_validate(symmetric=True).

Bars of the two NPR record fields, from the bar the suite already holds one eval-mode network to (tests/test_resunet_gpu.py:
relative L2 2e-5 against the oracle): the generator's unit 12-vectors carry its own 2e-5 and the encoder's 2e-5 handed on, so
an offset (0.3 x a unit 3-vector share) is off by dp <= 0.3 * 4e-5 = 1.2e-5 m.  The regulariser mean |offset|^2 then moves by
at most 2 * 4e-5 = 8e-5 of itself; a Chamfer term mean |p - q|^2 by 2 dp / d of itself, with d >= 0.1 m the stand-in clouds'
jitter, = 2.4e-4.  ReLU decisions and arg-mins are the oracle's own here: both terms are continuous in them.
Measured on an MI355X: Chamfer term 7.3e-8 / 8.2e-8 (strict / not), regulariser 1.2e-7 (L2), 2.1e-8 / 7.1e-9 (RepelL1)."""
import numpy as np
import pytest
import torch

from apr_amd import ops, synth
from apr_amd.fcgf.lib.learned import train_and_validate
from apr_amd.fcgf.lib.validation import SymmetricPairValidStep
from oracle import apr_step_oracle as AO
from oracle import me_oracle as OME
from tests.helpers import model_pair

pytestmark = pytest.mark.gpu
VS, RATIO = 0.3, 4
BAR_REG, BAR_CHAMFER = 8e-5, 2.4e-4


def _pair(dev, seed):
    """tests/test_valid_epoch_gpu.py's small pair (validation keys pcd0 / pcd1 / T_gt, stand-in APG clouds) at 8 x 200 rays."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=8, n_azimuth=200)
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
        out[f"pcd_nghb{tag}"] = [(p.repeat(2, 1) + jit).contiguous()]
    out["T_gt"] = torch.from_numpy(T).float()
    out["len_batch"] = [[int(out["sinput0_C"].shape[0]), int(out["sinput1_C"].shape[0])]]
    return out


@pytest.fixture(scope="module")
def chain(dev):
    """One small pair, the HIP models and the oracle generator's eval-mode output per frame (float64), computed once."""
    pair = _pair(dev, 3)
    oe, enc = model_pair("ResUNetFatBN", out_channels=128)
    og, gen = model_pair("ResUNetFatBN", out_channels=RATIO * 3, seed=1, in_channels=128)
    oe, og = oe.double().eval(), og.double().eval()
    G = []
    with torch.no_grad():
        for k in ("0", "1"):
            C = pair[f"sinput{k}_C"].cpu().numpy()
            x = OME.SparseTensor(torch.ones(len(C), 1, dtype=torch.float64), coordinates=C)
            G.append(og(oe(x)).F * VS)
    return pair, enc, gen, G


def _oracle_terms(pair, G, reg_type, strict):
    reg = cham = 0
    for k in (0, 1):
        term = AO.regulariser(G[k], reg_type, 0.1)
        reg = term if (reg_type == 'RepelL1' and strict) else reg + term
        xyz = pair[f"sinput{k}_C"][:, 1:].cpu().double()
        pts = (G[k] + VS * xyz.repeat(1, RATIO)).reshape(-1, 3)
        cham = cham + AO.chamfer(pts, pair["pcd_nghb0" if strict else f"pcd_nghb{k}"][0].cpu().double())[0]
    return float(cham / 2), float(reg / 2)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("reg_type", ["L2", "RepelL1"])
def test_npr_record_fields_match_the_oracle_chain(dev, chain, reg_type, strict):
    pair, enc, gen, G = chain
    step = SymmetricPairValidStep(enc, gen, voxel_size=VS, point_generation_ratio=RATIO, regularization_type=reg_type,
                                  subsample_size=500, strict_reference=strict)
    rec = torch.zeros((1, ops.VALID_RECORD_FLOATS), device=dev)
    enc.train()
    gen.eval()
    np.random.seed(0)
    step(pair, rec, 0)
    assert enc.training and not gen.training                    # left in the mode they were in
    r = rec.cpu().numpy()[0]
    cham, reg = _oracle_terms(pair, G, reg_type, strict)
    e_c, e_r = abs(float(r[ops.VALID_CHAMFER]) - cham) / cham, abs(float(r[ops.VALID_REG]) - reg) / reg
    print(f"[{reg_type} strict={strict}] chamfer {r[ops.VALID_CHAMFER]:.6f} vs {cham:.6f} ({e_c:.1e}); "
          f"regulariser {r[ops.VALID_REG]:.6f} vs {reg:.6f} ({e_r:.1e})")
    assert r[ops.VALID_N_CORR] == 500
    assert e_c <= BAR_CHAMFER and e_r <= BAR_REG


def test_strict_reference_changes_only_what_it_names(dev, chain):
    """Frame 1 against pcd_nghb0 or pcd_nghb1: another Chamfer term, the same L2 regulariser bits."""
    pair, enc, gen, _ = chain
    out = []
    for strict in (True, False):
        step = SymmetricPairValidStep(enc, gen, voxel_size=VS, point_generation_ratio=RATIO, subsample_size=500,
                                      strict_reference=strict)
        rec = torch.zeros((1, ops.VALID_RECORD_FLOATS), device=dev)
        np.random.seed(0)
        step(pair, rec, 0)
        out.append(rec.cpu().numpy()[0])
    assert out[0][ops.VALID_REG] == out[1][ops.VALID_REG] and out[0][ops.VALID_CHAMFER] != out[1][ops.VALID_CHAMFER]
    assert out[0][:ops.VALID_CHAMFER].tobytes() == out[1][:ops.VALID_CHAMFER].tobytes()


def test_reduced_symmetric_run_repeats_bit_for_bit_and_lowers_the_chamfer_term(dev):
    kw = dict(n_train=2, n_val=1, iterations=36, model="ResUNetFatBN", n_out=128, n_beams=8, n_azimuth=200, seed=0, k=1,
              lr=0.05, num_pos=256, num_hn=128, register=False, symmetric=True)
    a = train_and_validate(dev, **kw)
    b = train_and_validate(dev, **kw)
    print(f"seconds {a['seconds']}; chamfer {a['valid_before']['chamfer_distance']:.5f} -> {a['valid_after']['chamfer_distance']:.5f}; "
          f"loss {a['losses'][0]:.4f} -> {a['losses'][-1]:.4f}")
    assert a["losses"] == b["losses"] and len(a["losses"]) == 36 and all(np.isfinite(a["losses"]))
    assert a["records_after"].tobytes() == b["records_after"].tobytes()
    assert a["valid_after"]["chamfer_distance"] < a["valid_before"]["chamfer_distance"]
