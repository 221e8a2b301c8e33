"""ORACLE CHAIN of the symmetric APR training iteration (test infrastructure only), composed from the committed oracles:

  * oracle encoder (`resunet_oracle`), frame 0 then frame 1, as two separate calls     FCGF_APR/lib/complement_trainer.py:386-394
  * `match_pose_oracle.hardest_contrastive`                                            :398-409
  * oracle `ResUNetFatBN(n_out, ratio * 3)` as generator ON THE ENCODER'S TENSOR, frame 0 then frame 1    :413-419, :52-60
  * per frame, per cloud: the cloud's rows of the generator's output x voxel size      :427-428, :459-460
    -> `apr_step_oracle.regulariser` / generated points / `apr_step_oracle.chamfer`    :432-448
  * one backward, one `torch.optim.SGD` step over (encoder, generator)                 :485, :492

in whatever dtype the models hold (float64 for the tests).  Decisions can be pinned as in `apr_step_oracle`: `pins.enc` the
encoder's ReLU masks per frame, `gen_pins` the generator's per frame (same format: {node name: (coords, mask)}),
`pins.hardest`, `pins.chamfer`.
"""
import numpy as np
import torch

from oracle import apr_step_oracle as AO
from oracle import match_pose_oracle as MO
from oracle import me_oracle as OME
from oracle import resunet_oracle as OR


def generator_copy(name, state, n_in, n_out, dtype=torch.float64):
    """The oracle sparse generator `name`(n_in, n_out) in `dtype` on the CPU with the given (HIP) state_dict, train mode."""
    om = OR.MODELS[name](n_in, n_out, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    om.load_state_dict({k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in state.items()})
    return om.to(dtype).train()


def encode(encoder, coords, feats, pins=None):
    """Both encoder calls -> the two output SparseTensors (their F retains its gradient)."""
    dtype = next(encoder.parameters()).dtype
    out = []
    for k in range(2):
        x = OME.SparseTensor(torch.as_tensor(feats[k]).to(dtype), coordinates=np.asarray(coords[k]))
        y = encoder(x, pins[k] if pins else None)
        if y.F.requires_grad:
            y.F.retain_grad()
        out.append(y)
    return out


def npr_terms(gens, coords, clouds, cfg, chamfer_pins=None):
    """Per frame, per cloud (:424-449, :455-481 with the symmetric lines): -> (chamfer terms, regulariser terms, arg-mins)."""
    dtype = gens[0].F.dtype
    cham, reg, argmin, call = [], [], [], 0
    for k in range(2):
        C = np.asarray(coords[k])
        for i, (s, e) in enumerate(AO.cloud_rows(C)):
            generated = gens[k].F[s:e] * cfg.voxel_size
            reg.append(AO.regulariser(generated, cfg.reg_type, cfg.alpha))
            xyz = torch.from_numpy(C[s:e, 1:].astype(np.float64)).to(dtype)
            mod = (generated + cfg.voxel_size * xyz.repeat(1, cfg.ratio)).reshape(-1, 3)
            c, am = AO.chamfer(mod, torch.as_tensor(clouds[k][i]).to(dtype), chamfer_pins[call] if chamfer_pins else None)
            cham.append(c)
            argmin.append(am)
            call += 1
    return cham, reg, argmin


def iteration(encoder, generator, coords, feats, clouds, positive_pairs, draws, cfg: AO.StepConfig, pins: AO.Pins = None,
              gen_pins=None):
    """The forward half of one symmetric iteration -> apr_step_oracle.Iteration (its `loss` not yet back-propagated)."""
    pins = pins or AO.Pins()
    it = AO.Iteration()
    enc = encode(encoder, coords, feats, pins.enc)
    it.F = [y.F for y in enc]
    sel0, sel1, pos_sel = draws
    it.pos_loss, it.neg_loss = MO.hardest_contrastive(it.F[0], it.F[1], positive_pairs, sel0, sel1, pos_sel, cfg.pos_thresh,
                                                      cfg.neg_thresh, hardest=pins.hardest)
    loss = it.pos_loss + cfg.neg_weight * it.neg_loss
    gens = [generator(enc[k], gen_pins[k] if gen_pins else None) for k in range(2)]      # frame 0, then frame 1
    it.cham, it.reg, it.argmin = npr_terms(gens, coords, clouds, cfg, pins.chamfer)
    for c, r in zip(it.cham, it.reg):
        loss = loss + (c + r * cfg.reg_strength) * cfg.loss_ratio
    it.loss = loss
    return it


def step(encoder, generator, optimizer, *args, **kw):
    """zero_grad -> iteration -> backward -> optimizer.step() -> the Iteration."""
    optimizer.zero_grad()
    it = iteration(encoder, generator, *args, **kw)
    it.loss.backward()
    optimizer.step()
    return it
