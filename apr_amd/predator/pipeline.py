"""One scan pair through the Predator_APR hot path on the GPU: grid subsample -> KPConv index pyramid ->
KPFCNN (encoder + overlap attention + decoder) -> score-weighted sampling -> RANSAC/SVD.

This is the per-pair body of the reference's tester (Predator_APR/lib/tester.py:48-110) with its data-loader work
(datasets/kitti.py:466-471 voxel_down_sample, datasets/dataloader.py collate_fn_descriptor) pulled onto the device.
The counterpart of apr_amd.fcgf.pipeline.PairRegistration.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _host
from . import point_ops
from .datasets.dataloader import calibrate_neighbors, collate_fn_descriptor   # noqa: F401  (re-exported)
from .lib import benchmark_utils as BU


_DRAW_POOL = None


def _draw_pool():
    """One helper thread per process for the host-RNG draws (see register_batch_phases)."""
    global _DRAW_POOL
    if _DRAW_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _DRAW_POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="apr-draw")
    return _DRAW_POOL


class HostPending:
    """A host job in flight on a helper thread, with the face of ops.PendingFetch: `.event.query()` / `.wait()` / `.finish()`
    (apr_amd.fcgf.pipeline.run_pipelined and ops.drive treat both alike)."""

    def __init__(self, future):
        self._future = future
        self.event = self

    def query(self):
        return self._future.done()

    def synchronize(self):
        self._future.result()

    def wait(self, mode=None):
        self._future.result()

    def finish(self):
        return self._future.result()


class PredatorRegistration:
    def __init__(self, model, config, neighborhood_limits, voxel_size=0.3, n_points=5000, distance_threshold=0.3,
                 max_iteration=50000, max_validation=1000, voxelizer='grid'):
        """`neighborhood_limits`: per-level caps of the radius neighbourhoods (the reference calibrates them once per
        dataset, datasets/dataloader.py:calibrate_neighbors); `n_points`: interest points kept per frame
        (configs/test/kitti.yaml n_points); `voxelizer`: 'grid' feeds the network the barycentres of apr_grid_subsample
        (the grid of the KPConv pyramid), 'open3d' the centroids of the loader's own voxel_down_sample
        (datasets/kitti.py:588-589; apr_voxel_down_sample, rounded to fp32 once)."""
        _host.limit_cpu_threads()
        if voxelizer not in ('grid', 'open3d'):
            raise ValueError(f"PredatorRegistration: voxelizer must be 'grid' or 'open3d', got {voxelizer!r}")
        self.voxelizer = voxelizer
        self.model = model.eval()
        self.config = config
        self.limits = list(neighborhood_limits)
        self.voxel_size = float(voxel_size)
        self.n_points = int(n_points)
        self.distance_threshold = float(distance_threshold)
        self.max_iteration, self.max_validation = int(max_iteration), int(max_validation)

    def _voxelise(self, points, lens):
        """-> (fp32 points of the voxelised clouds, their lengths) by the configured voxelizer."""
        if self.voxelizer == 'open3d':
            from .. import ops
            out, sub = ops.voxel_down_sample(points, lens, self.voxel_size, want=("centroid32",))
            return out["centroid32"], sub
        return point_ops.grid_subsample(points, lens, self.voxel_size)

    @torch.no_grad()
    def encode(self, xyz0, xyz1):
        """-> (src points, tgt points, features [n0+n1, C], overlap scores, saliency scores)."""
        dev = xyz0.device
        lens = np.array([len(xyz0), len(xyz1)], np.int32)
        pts, lens = self._voxelise(torch.cat([xyz0, xyz1]), lens)
        src, tgt = pts[:lens[0]], pts[lens[0]:]
        ones = lambda p: torch.ones((len(p), 1), device=dev)
        batch = collate_fn_descriptor([(src, tgt, ones(src), ones(tgt))], self.config, self.limits)
        feats, overlap, saliency = self.model(batch)
        return src, tgt, feats, overlap, saliency

    @torch.no_grad()
    def encode_batch(self, pairs):
        """Several pairs through ONE collate and ONE network forward (their clouds stacked at every level; see
        `collate_fn_descriptor`).  -> per pair (src points, tgt points, features, overlap, saliency), each what
        `encode` returns for that pair alone."""
        dev = pairs[0][0].device
        clouds = [c for pair in pairs for c in pair]
        lens = np.array([len(c) for c in clouds], np.int32)
        pts, lens = self._voxelise(torch.cat(clouds), lens)
        ends = np.cumsum(lens)
        sub = [pts[e - n:e] for e, n in zip(ends, lens)]
        ones = lambda p: torch.ones((len(p), 1), device=dev)
        items = [(sub[2 * i], sub[2 * i + 1], ones(sub[2 * i]), ones(sub[2 * i + 1])) for i in range(len(pairs))]
        feats, overlap, saliency = self.model(collate_fn_descriptor(items, self.config, self.limits))
        out = []
        for i in range(len(pairs)):
            a, b = int(ends[2 * i] - lens[2 * i]), int(ends[2 * i + 1])
            out.append((sub[2 * i], sub[2 * i + 1], feats[a:b], overlap[a:b], saliency[a:b]))
        return out

    @torch.no_grad()
    def register_batch(self, pairs, seeds=None):
        """[(xyz0, xyz1), ...] -> [(T, info), ...]: one stacked encode, then the reference's per-pair tail
        (lib/tester.py:80-100: score-weighted draws on the host RNG seeded per pair, feature NN, RANSAC)."""
        from .. import ops
        return ops.drive(self.register_batch_phases(pairs, seeds))     # one code path: the pipelined batch, waited for

    @torch.no_grad()
    def register_batch_phases(self, pairs, seeds=None):
        """`register_batch` as a generator for a single-thread scheduler (apr_amd.fcgf.pipeline.run_pipelined): every
        place where the blocking form waits for bytes from the device -- the cloud lengths after each grid subsample
        (1 + 4 per batch), the neighbour-table widths, the sampling weights, the RANSAC results -- yields an
        ops.PendingFetch instead; all device work goes to the CURRENT stream.  Returns [(T, info), ...]."""
        from .. import ops
        seeds = list(range(len(pairs))) if seeds is None else list(seeds)
        dev = pairs[0][0].device
        clouds = [c for pair in pairs for c in pair]
        if self.voxelizer == 'open3d':      # apr_voxel_down_sample has no synchronisation-free form
            pts, lens = self._voxelise(torch.cat(clouds), np.array([len(c) for c in clouds], np.int32))
        else:
            sub0 = point_ops.grid_subsample_async(torch.cat(clouds), np.array([len(c) for c in clouds], np.int32),
                                                  self.voxel_size)
            yield sub0.fetch
            pts, lens = sub0.finish()
        ends = np.cumsum(lens)
        sub = [pts[e - n:e] for e, n in zip(ends, lens)]
        ones = lambda p: torch.ones((len(p), 1), device=dev)
        items = [(sub[2 * i], sub[2 * i + 1], ones(sub[2 * i]), ones(sub[2 * i + 1])) for i in range(len(pairs))]
        raws, n01 = yield from self._match_phases(items, seeds, None)
        rfetch = ops.PendingFetch(torch.stack(raws), lambda host: host.copy())
        yield rfetch
        out = []
        for raw, (n0, n1, ns) in zip(rfetch.finish(), n01):
            T, info = ops.ransac_decode(raw, ns)
            info.update(n0=n0, n1=n1)
            out.append((T, info))
        return out

    def _match_phases(self, items, seeds, draws, after=None):
        """The tail that `register_batch_phases` and `register_samples_phases` share, from the voxelised clouds on:
        collate, network, the score-weighted draws (lib/tester.py:80-92), feature NN and the RANSAC enqueue of every pair.
        `items`: per pair (src, tgt, src_feats, tgt_feats, ...) as the collate takes them; the clouds that are sampled and
        registered are the items' raw clouds where they have them (index 7, 8: `inputs['src_pcd_raw']`), else the inputs.
        `draws`: None -- pair i draws from its own `np.random.RandomState(seeds[i])`; a `RandomState` or the `np.random`
        module -- every pair draws from that one stream, source then target, in pair order.  `after(i, s_p, t_p, corr,
        raw)` runs right behind pair i's RANSAC enqueue.  -> (raw results on the device, [(n0, n1, ns), ...])."""
        from .. import ops
        from .datasets.dataloader import collate_phases
        f32 = lambda p: p.to(torch.float32).contiguous()
        clouds = [(f32(it[7]), f32(it[8])) if len(it) > 8 else (it[0], it[1]) for it in items]
        batch = yield from collate_phases([tuple(it[:4]) for it in items], self.config, self.limits)
        feats, overlap, saliency = self.model(batch)
        wfetch = ops.PendingFetch(overlap * saliency, lambda host: host.copy())
        yield wfetch
        w_all = torch.from_numpy(wfetch.finish())
        # the score-weighted draws of all pairs (NumPy's legacy choice on each pair's own RandomState: 0.39 ms of host time
        # per pair, most of it inside the library's host function, which releases the GIL) run on a helper thread while the
        # scheduler thread serves the other batches
        spans, a = [], 0
        for it in items:
            spans.append((a, len(it[0]), len(it[1])))
            a += len(it[0]) + len(it[1])

        def draw_all():
            out_ = []
            for (a, n0, n1), seed in zip(spans, seeds):
                rng = np.random.RandomState(seed) if draws is None else draws
                i0 = BU.draw_by_score(n0, w_all[a:a + n0], self.n_points, rng)
                i1 = BU.draw_by_score(n1, w_all[a + n0:a + n0 + n1], self.n_points, rng)
                out_.append((i0, i1))
            return out_

        dfetch = HostPending(_draw_pool().submit(draw_all))
        yield dfetch
        drawn = dfetch.finish()
        raws, n01 = [], []
        for i, seed in enumerate(seeds):
            a, n0, n1 = spans[i]
            b = a + n0 + n1
            s_p, s_f = BU.take_drawn(clouds[i][0], feats[a:a + n0], drawn[i][0])
            t_p, t_f = BU.take_drawn(clouds[i][1], feats[a + n0:b], drawn[i][1])
            corr = ops.feature_nn(s_f.contiguous(), t_f.contiguous())
            raws.append(ops.ransac_pose_geometric_async(s_p, t_p, corr, self.distance_threshold, 0.9, self.max_iteration,
                                                        self.max_validation, seed))
            n01.append((n0, n1, len(s_p)))
            if after is not None:
                after(i, s_p, t_p, corr, raws[-1])
        return raws, n01

    @torch.no_grad()
    def register_samples_phases(self, items, draws=None, seeds=None, records=None, slot0=0, rot_threshold=5,
                                trans_threshold=2, inlier_distance_threshold=0.1):
        """The tail of `register_batch_phases` for clouds the loader already voxelised: `items` are
        `datasets.kitti.test_sample` / `training_sample` tuples (or any (src, tgt, src_feats, tgt_feats, rot, trans, ...)),
        no voxeliser call is made.  Behind each pair's RANSAC enqueue, `ops.predator_test_pair` turns the raw result into
        row `slot0 + i` of `records` (float64 [pairs, 32] on the GPU, columns `ops.PTEST_*`; None: a buffer of len(items)
        rows): no raw result travels to the host, the caller reads `records` once when its epoch is over.
        `draws` / `seeds`: see `_match_phases`; `seeds` are the RANSAC seeds too (default: the pair index).
        Returns `records`."""
        from .. import ops
        items = list(items)
        seeds = list(range(len(items))) if seeds is None else list(seeds)
        if len(seeds) != len(items):
            raise ValueError(f"register_samples: {len(items)} pairs but {len(seeds)} seeds")
        dev = items[0][0].device
        if records is None:
            records = torch.zeros((slot0 + len(items), ops.PTEST_RECORD_FLOATS), dtype=torch.float64, device=dev)
        gt = [(it[4].to(dev, torch.float32).reshape(3, 3).contiguous(), it[5].to(dev, torch.float32).reshape(3).contiguous())
              for it in items]

        def after(i, s_p, t_p, corr, raw):
            ops.predator_test_pair(s_p, t_p, corr, gt[i][0], gt[i][1], raw, records, slot0 + i,
                                   distance_threshold=self.distance_threshold,
                                   inlier_distance_threshold=inlier_distance_threshold, rot_threshold=rot_threshold,
                                   trans_threshold=trans_threshold)

        yield from self._match_phases(items, seeds, draws, after)
        return records

    @torch.no_grad()
    def register_samples(self, items, draws=None, seeds=None, **kw):
        """`register_samples_phases`, waited for -> the records on the host (float64 [pairs, 32]), fetched once."""
        from .. import ops
        return ops.drive(self.register_samples_phases(items, draws, seeds, **kw)).cpu().numpy()

    @torch.no_grad()
    def __call__(self, xyz0, xyz1, seed=0):
        src, tgt, feats, ov, sal = self.encode(xyz0, xyz1)
        n0 = len(src)
        rng = np.random.RandomState(seed)
        s_p, s_f, _ = BU.sample_by_score(src, feats[:n0], ov[:n0] * sal[:n0], self.n_points, rng=rng)
        t_p, t_f, _ = BU.sample_by_score(tgt, feats[n0:], ov[n0:] * sal[n0:], self.n_points, rng=rng)
        T, info = BU.ransac_pose_estimation(s_p, t_p, s_f, t_f, distance_threshold=self.distance_threshold, ransac_n=4,
                                            max_iteration=self.max_iteration, max_validation=self.max_validation,
                                            seed=seed, return_info=True)
        info.update(n0=n0, n1=len(tgt))
        return T, info
