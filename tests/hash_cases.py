"""Named inputs for voxel hashing, coordinate maps and kernel maps (apr_amd/csrc/hash.hip, apr_voxel_pyramid in
encoder.hip), each with the fact it plants; tests/test_hash_oracle_cpu.py confirms every fact on the host.  numpy only,
everything from small integer seeds.

Kernel constants the cases are built around:
* rows are (batch, x, y, z) with 0 <= batch < 1023 and -2^17 <= x, y, z < 2^17 (common.h); a live row outside sets the
  build's status word, a probe outside finds nothing.
* apr_map_build: one thread per row, 256 per block, 64 per wave.  k_insert: inside a wave the first lane of a run of equal
  keys probes, the others take its slot by shuffle; an out-of-range or dead lane starts a run of its own.  k_scan_blocks:
  ONE workgroup of 1024 threads scans the per-block counts, 1024 blocks per trip with a carry between trips: a second
  trip needs more than 1024 * 256 = 262 144 rows.
* the table has apr_hash_capacity(n) = max(1024, first power of two >= 2n) slots, home slot = murmur3 finaliser of the
  packed key & (cap - 1), linear probing.
* k_kernel_map / k_kernel_map_sym: one thread per (row, offset) probe, at most 65 536 blocks of 256, grid stride beyond;
  the symmetric kernel probes K / 2 + 1 offsets per row and k_fill_upper (-1 into the upper half) has at most 16 384
  blocks.
* k_fill_bytes: 16-byte stores behind an unaligned head of (16 - phase) % 16 bytes, at most 2048 blocks of 256 threads,
  8 stores per thread before the cap binds.  k_pack_i32: at most 64 blocks of 256 threads.
* apr_voxel_pyramid: above 262 144 points the unique voxels are re-inserted into a compact table of
  R = max(N / 4, 65 536) rows; more than R voxels is reported as a fallback.
"""
import numpy as np

import hash_oracle as O

F32 = np.float32
LO, HI = O.AXIS_LO, O.AXIS_HI
BLOCK, WAVE = 256, 64
SCAN_TRIP_ROWS = 1024 * BLOCK
KMAP_GRID_THREADS = 65536 * 256
FILL_UPPER_BLOCKS = 16384
FILL_8_PER_THREAD = 2048 * 256 * 16            # 2048 blocks x 256 threads x one 16-byte store: 8 388 608 bytes
FILL_GRID_BYTES = 2048 * 2048 * 16             # above this nblk is capped at 2048 and the stride loop takes a ninth trip
PACK_GRID_WORDS = 64 * 256
MAX_FRAMES = 64
COMPACT_ABOVE = 4 * 65536
VOXEL_SIZES = (0.3, 0.05, 0.25)                # the two the configs use (encoder, ICP) and a power of two
EMPTY = -1                                     # APR_KEY_EMPTY read as int64


def compact_rows(n_points):
    return max(n_points // 4, 65536) if n_points > COMPACT_ABOVE else 0


# ------------------------------------------------------------------------------------------------- the library's hash
def pack_key(b, x, y, z):
    """Python copy of apr_pack_key (only to CHOOSE rows by their home slot; never used to check a result)."""
    return (((int(b) << 18 | (int(x) + HI)) << 18 | (int(y) + HI)) << 18) | (int(z) + HI)


def hash_u64(k):
    m = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & m
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & m
    k ^= k >> 33
    return k & 0xFFFFFFFF


def home(row, cap):
    return hash_u64(pack_key(*row)) & (cap - 1)


def simulate_table(rows, cap):
    """Slots occupied after inserting `rows` by linear probing (the SET of occupied slots does not depend on the order)."""
    occ = [False] * cap
    for r in rows:
        s = home(r, cap)
        while occ[s]:
            s = (s + 1) & (cap - 1)
        occ[s] = True
    return np.array(occ)


# ------------------------------------------------------------------------------------------------- voxelisation values
def _quot_floor(x, vs):
    return np.floor(np.asarray(x, F32) / F32(vs))


def range_edge(vs, sign):
    """(largest-magnitude float32 of this sign whose voxel index is still in range, the first one whose index is not)."""
    x = F32(sign * float(HI) * vs)
    inside = lambda v: LO <= float(_quot_floor(v, vs)) < HI      # noqa: E731
    away = F32(np.inf * sign)
    while inside(x):
        x = np.nextafter(x, away)
    while not inside(x):
        x = np.nextafter(x, F32(0))
    return F32(x), F32(np.nextafter(x, away))


def voxel_values(vs):
    """-> dict(inside f32 [n, 3], outside f32 [m, 3], denormal f32 [2]).  `inside`: every planted value on every axis;
    `outside`: one row per (first out-of-range value, axis), the other two axes benign."""
    v = []
    for k in (1, 2, 3, 7, 10, 100, 1000, 4097, 65536, 131071):
        for s in (1, -1):
            x = F32(F32(s * k) * F32(vs))                       # the float32 multiple
            v += [x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))]
            x = F32(s * k * vs)                                 # the multiple rounded once from float64
            v += [x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))]
    den = [F32(-1e-45), F32(-1e-40)]
    v += [F32(0.0), F32(-0.0)] + den
    v += [np.nextafter(F32(0), F32(1)), F32(np.finfo(F32).tiny), -F32(np.finfo(F32).tiny)]
    (pin, pout), (nin, nout) = range_edge(vs, 1), range_edge(vs, -1)
    v += [pin, nin]
    v = np.array(v, F32)
    v = v[(_quot_floor(v, vs) >= LO) & (_quot_floor(v, vs) < HI)]      # +-131071 steps may leave the range: dropped here
    m = len(v)
    inside = np.stack([v, np.roll(v, 1), np.roll(v, 2)], 1)
    outside = []
    for x in (pout, nout):
        for a in range(3):
            row = [F32(0.5 * vs)] * 3
            row[a] = x
            outside.append(row)
    return dict(vs=vs, inside=inside, outside=np.array(outside, F32), denormal=np.array(den, F32), edges=(pin, pout, nin, nout),
                n_values=m)


# ------------------------------------------------------------------------------------------------- map-build row patterns
def _box_rows(rng, n, side=12, b=0, replace=False):
    """n rows drawn from the cube [-side/2, side/2)^3 of batch b."""
    ids = rng.choice(side ** 3, n, replace=replace)
    h = side // 2
    return np.stack([np.full(n, b), ids % side - h, (ids // side) % side - h, ids // (side * side) - h], 1).astype(np.int32)


def _case(name, fact, rows, floor_to=0, n_live=None, **kw):
    return dict(name=name, fact=fact, rows=np.ascontiguousarray(rows, np.int32).reshape(-1, 4), floor_to=floor_to,
                n_live=n_live, **kw)


def _with_run(rng, n, start, length, key=(0, 40, 41, 42)):
    rows = _box_rows(rng, n, 12)
    rows[start:start + length] = key
    return rows


OOR_ROWS = {"x": (0, HI, 0, 0), "z": (0, 0, 0, LO - 1), "b": (1023, 0, 0, 0)}


def map_cases():
    c = {}

    def add(*a, **k):
        d = _case(*a, **k)
        c[d["name"]] = d

    for n in (1, 63, 64, 65, 255, 256, 257):
        add(f"rows_{n}", f"{n} rows, about two per voxel, duplicates scattered", _box_rows(np.random.default_rng(n), n, 5, replace=True))
    rng = np.random.default_rng(1)
    add("run_cross_wave", "a run of 8 equal rows at 60 .. 67 (lanes 60 .. 63 of wave 0, 0 .. 3 of wave 1)", _with_run(rng, 200, 60, 8),
        run=(60, 8))
    add("run_cross_block", "a run of 12 equal rows at 250 .. 261 (blocks 0 and 1)", _with_run(rng, 400, 250, 12), run=(250, 12))
    add("run_longer_than_wave", "a run of 150 equal rows at 30 .. 179 (three waves)", _with_run(rng, 300, 30, 150), run=(30, 150))
    rows = _with_run(rng, 100, 10, 7)
    rows[13] = OOR_ROWS["x"]
    add("run_oor_middle", "A A A X A A A at 10 .. 16 in one wave, X out of range", rows, run=(10, 7), oor=13)
    rows = _box_rows(rng, 100, 12)
    A, B = (0, 40, 41, 42), (0, 40, 41, 43)
    rows[5:8] = [A, B, A]
    rows[20:26] = [A, A, B, B, A, A]
    add("aba_one_wave", "A B A at 5 .. 7 and A A B B A A at 20 .. 25 of wave 0", rows, aba=(5, 20))
    add("all_equal", "300 equal rows", np.tile(np.array([[3, -7, 9, -11]], np.int32), (300, 1)))
    add("all_distinct", "300 distinct rows", _box_rows(rng, 300, 12))
    corners = [(b, x, y, z) for b in (0, 1022) for x in (LO, HI - 1) for y in (LO, HI - 1) for z in (LO, HI - 1)]
    add("range_corners", "the eight corners of the range under batch 0 and 1022, each twice", np.array(corners + corners[::-1], np.int32))
    for ax, row in OOR_ROWS.items():
        rows = _box_rows(rng, 70, 12)
        rows[37] = row
        add(f"oor_{ax}", f"one row just outside the range: {row}", rows, oor=37)
    vals = np.array([-1, -2, -7, -8, -9, 0, 1, 2, 7, 8, 9, LO + 1, HI - 1], np.int32)
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    g = np.concatenate([np.zeros((len(g), 1), np.int32), g], 1)[np.random.default_rng(2).permutation(len(g))]
    for f in (2, 4, 8):
        add(f"floor_to_{f}", f"coordinates -1 -2 -7 -8 -9 0 1 2 7 8 9 -2^17+1 2^17-1 on every axis, floored to {f}", g, floor_to=f)

    def tail_filled(seed, n, n_live, run=None):
        r = np.random.default_rng(seed)
        rows = _box_rows(r, n, 6, replace=True)
        if run:
            rows[run[0]:run[0] + run[1]] = (0, 40, 41, 42)
        t = np.arange(n_live, n)
        rows[t[0::2]] = OOR_ROWS["x"]                                                  # garbage the build must not see
        if n_live > 0:
            rows[t[1::2]] = rows[r.integers(0, n_live, len(t[1::2]))]                  # copies of live rows
        else:
            rows[t[1::2]] = (0, 1, 2, 3)
        return rows
    add("live_cuts_run", "n_live = 305 inside the run 300 .. 309; rows past it: out of range / copies of live rows",
        tail_filled(3, 600, 305, (300, 10)), n_live=305, run=(300, 10))
    add("live_block_edge", "n_live = 512 = two whole blocks of 700 rows", tail_filled(4, 700, 512), n_live=512)
    add("live_zero", "n_live = 0 of 300 rows", tail_filled(5, 300, 0), n_live=0)
    return c


def scan_two_trips():
    """262 145 rows = 1025 blocks: the smallest count that gives k_scan_blocks a second trip.  About 3 rows per voxel: runs
    of 1 or 2 equal rows, and the voxels come back later (~175 000 runs drawn from the 110 592 cells of a 48^3 box fill
    ~88 000 of them).  The last row is a voxel of its own, so the lone block of the second trip holds a first occurrence
    that needs the carry."""
    n = SCAN_TRIP_ROWS + 1
    rng = np.random.default_rng(7)
    runs = rng.integers(1, 3, n)
    ids = np.repeat(rng.integers(0, 48 ** 3, len(runs)), runs)[:n]
    assert len(ids) == n
    rows = np.stack([np.zeros(n, np.int64), ids % 48 - 24, (ids // 48) % 48 - 24, ids // 2304 - 24], 1).astype(np.int32)
    rows[-1] = (1, 0, 0, 0)
    return _case("scan_two_trips", "1025 blocks; the last row is a new voxel", rows)


# ------------------------------------------------------------------------------------------------- probe wrap
WRAP_CAP = 1024


def probe_wrap():
    """296 rows -> 1024 slots.  40 rows have their home among the last four slots, so by pigeonhole their chain runs
    through slot 1023 into slots 0 .. 35 at least.  12 ABSENT coordinates with the same homes sit at x - 1 of a present
    row: that row's probe at offset (-1, 0, 0) misses after walking the chain across the wrap."""
    cand = [(0, x, y, z) for x in range(-30, 30, 2) for y in range(-30, 30) for z in range(-30, 30)      # even x only ...
            if home((0, x, y, z), WRAP_CAP) >= WRAP_CAP - 4]
    assert len(cand) >= 52
    rng = np.random.default_rng(9)
    rng.shuffle(cand)
    chain, absent = cand[:40], cand[40:52]
    partners = [(0, x + 1, y, z) for (_, x, y, z) in absent]                                             # ... odd x: never a candidate
    rest = [tuple(int(v) for v in r) for r in _box_rows(rng, 400, 60)]
    seen, rows = set(absent), []
    for r in chain + partners + rest:
        if r not in seen and len(rows) < 296:
            seen.add(r)
            rows.append(r)
    rows = np.array(rows, np.int32)[rng.permutation(len(rows))]
    return dict(name="probe_wrap", fact="40 homes in slots 1020 .. 1023, 12 absent probes with the same homes", rows=rows,
                chain=np.array(chain, np.int32), absent=np.array(absent, np.int32), cap=WRAP_CAP)


# ------------------------------------------------------------------------------------------------- kernel maps
def _dense_rows(seed, n, dims, scale=1, batches=(0,)):
    """n distinct rows, multiples of `scale`, from a box of dims cells centred on 0, per batch; shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    for b in batches:
        ids = rng.choice(dims[0] * dims[1] * dims[2], n, replace=False)
        out.append(np.stack([np.full(n, b), (ids % dims[0] - dims[0] // 2) * scale, ((ids // dims[0]) % dims[1] - dims[1] // 2) * scale,
                             (ids // (dims[0] * dims[1]) - dims[2] // 2) * scale], 1))
    rows = np.concatenate(out).astype(np.int32)
    return rows[rng.permutation(len(rows))]


def _kcase(name, fact, rows, ks, scale, kind="same", **kw):
    """kind: same = out map is the in map (generic AND symmetric kernel); strided = out is the in map floored to 2 * scale;
    transposed = out is the fine map, in the floored one, probed with -scale."""
    return dict(name=name, fact=fact, rows=np.ascontiguousarray(rows, np.int32).reshape(-1, 4), ks=ks, scale=scale, kind=kind, **kw)


ALIAS_Z = [(0, 5, 7, HI - 1), (0, 5, 8, LO)]
ALIAS_B = [(0, HI - 1, 3, 3), (1, LO, 3, 3)]


def _face_rows(scale):
    """Rows on all six faces of the range, the two aliasing pairs, multiples of `scale`."""
    top, bot = HI - scale, LO
    rows = [(0, top, 0, 0), (0, bot, 0, 0), (0, 0, top, 0), (0, 0, bot, 0), (0, 0, 0, top), (0, 0, 0, bot),
            (0, top, top, top), (0, bot, bot, bot), (1, bot, top, bot), (1022, top, top, top), (1022, bot, bot, bot),
            (0, top - scale, 0, 0), (0, bot + scale, 0, 0), (0, 0, 0, top - scale), (0, 0, 0, bot + scale),
            (0, top, scale, 0), (0, bot, scale, 0), (0, top, scale, bot), (0, bot, 2 * scale, top)]
    if scale == 1:
        rows += ALIAS_Z + ALIAS_B
    return np.array(rows, np.int32)


def kernel_map_cases():
    c = {}

    def add(*a, **k):
        d = _kcase(*a, **k)
        c[d["name"]] = d

    for ks, n in ((3, 256), (3, 257), (5, 256), (5, 255), (7, 256), (7, 255)):
        K = ks ** 3
        add(f"k{ks}_n{n}", f"n * K = {n * K} is {'a' if n * K % 256 == 0 else 'no'} multiple of 256; a box half full", _dense_rows(ks * 1000 + n, n, (8, 8, 8)),
            ks, 1, occ=True)
    for s in (2, 4, 8):
        add(f"k3_scale{s}", f"a level at tensor stride {s}", _dense_rows(s, 200, (7, 8, 7), s), 3, s)
    add("k5_scale2", "5^3 at tensor stride 2", _dense_rows(52, 201, (8, 7, 8), 2), 5, 2)
    add("k7_scale8", "7^3 at tensor stride 8", _dense_rows(78, 130, (6, 7, 6), 8), 7, 8)
    for s in (1, 2, 4):
        add(f"strided_{s}_to_{2 * s}", f"fine level {s} to the level floored to {2 * s}; negative coordinates", _dense_rows(20 + s, 300, (9, 9, 9), s), 3, s,
            kind="strided", occ=s == 1)
        add(f"transposed_{2 * s}_to_{s}", f"fine rows probe the floored level with scale -{s}", _dense_rows(30 + s, 300, (9, 9, 9), s), 3, s,
            kind="transposed")
    add("one_row", "a map of one row", np.array([[0, 1, 2, 3]], np.int32), 3, 1)
    add("one_row_k7", "a map of one row, 343 probes", np.array([[5, -1, -2, -3]], np.int32), 7, 1)
    add("two_batches", "two items over the same 8^3 block: only the batch index separates neighbours", _dense_rows(40, 256, (8, 8, 8), 1, (0, 1)), 3, 1)
    add("two_batches_k5", "the same under 5^3 and far-apart batch indices", _dense_rows(41, 200, (8, 8, 8), 1, (7, 1022)), 5, 1)
    for ks in (3, 5, 7):
        add(f"range_faces_k{ks}", "rows on the faces of the range and the two aliasing pairs: probes leave the range", _face_rows(1), ks, 1)
    add("coarse_faces_k3", "a level at stride 8 on the faces: scale * offset = 8 steps across", _face_rows(8), 3, 8)
    add("coarse_faces_k7", "a level at stride 8 on the faces: scale * offset = 24 steps across", _face_rows(8), 7, 8)
    add("strided_faces", "stride 1 -> 2 on the faces", _face_rows(1), 3, 1, kind="strided")
    add("transposed_faces", "scale -1 on the faces", _face_rows(1), 3, 1, kind="transposed")
    return c


# 65 536 blocks of 256 threads cover 16 777 216 probes.  Generic kernel at 7^3: n * 343 > 16 777 216  <=>  n >= 48 914.
BIG_GENERIC_ROWS = KMAP_GRID_THREADS // 343 + 1
# Symmetric kernel at 7^3: K / 2 + 1 = 172 probes per row, n * 172 > 16 777 216  <=>  n >= 97 542; k_fill_upper then has
# n * 171 / 256 = 65 155 blocks' worth of entries, four times its cap of 16 384.
BIG_SYM_ROWS = KMAP_GRID_THREADS // 172 + 1


def big_generic():
    """48 914 of the 46 * 46 * 47 = 99 452 cells: density 0.49."""
    return _kcase("big_generic", "the smallest row count whose 7^3 probes exceed 65 536 blocks", _dense_rows(100, BIG_GENERIC_ROWS, (46, 46, 47)), 7, 1)


def big_sym():
    """97 542 of the 58^3 = 195 112 cells: density 0.50."""
    return _kcase("big_sym", "the smallest row count whose 172 probes per row exceed 65 536 blocks", _dense_rows(101, BIG_SYM_ROWS, (58, 58, 58)), 7, 1)


# ------------------------------------------------------------------------------------------------- transpose
def transpose_cases():
    """Forward tables nbr[j coarse, k] = i fine over a coarse map built from a SUBSET of the fine rows: fine rows whose
    parent was left out have no partner and an all -1 row in the transpose."""
    c = {}
    for seed, n, s in ((1, 300, 1), (2, 257, 2)):
        fine = _dense_rows(50 + seed, n, (9, 9, 9), s)
        coarse, _, _ = O.build_map(fine[: n // 3], floor_to=2 * s)
        c[f"subset_{s}"] = dict(nbr=O.kernel_map(coarse, fine, 3, s), n_in=n, fact="parents of two thirds of the fine rows left out")
    c["zero_rows"] = dict(nbr=np.zeros((0, 27), np.int32), n_in=5, fact="no forward rows: all -1")
    c["one_row"] = dict(nbr=np.array([[-1, 0, -1, 0, 0] + [-1] * 22], np.int32), n_in=1, fact="one forward row, one fine row")
    c["one_row_k125"] = dict(nbr=np.where(np.arange(125) % 3 == 0, np.arange(125) % 4, -1).astype(np.int32)[None], n_in=4,
                             fact="one forward row over four fine rows, K = 125")
    return c


# ------------------------------------------------------------------------------------------------- front end
def _cloud(rng, voxels, vs):
    """One point per given voxel (int [n, 3]), placed inside the voxel away from its faces."""
    v = np.asarray(voxels, np.float64).reshape(-1, 3)
    return ((v + rng.uniform(0.2, 0.8, v.shape)) * vs).astype(F32)


def _frame_voxels(rng, n, run=3, side=14):
    """n points as runs of `run` points per voxel over a small cube (voxels come back)."""
    ids = np.repeat(rng.integers(0, side ** 3, n // run + 1), run)[:n]
    return np.stack([ids % side - side // 2, (ids // side) % side - side // 2, ids // (side * side) - side // 2], 1)


def frame_cases(vs=0.3):
    c = {}
    rng = np.random.default_rng(21)

    def add(name, fact, sizes, shared_run=False):
        vox = [_frame_voxels(rng, n) for n in sizes]
        if shared_run:            # the run that straddles a frame boundary: same voxel, two frames -> two rows
            nz = [i for i, n in enumerate(sizes) if n > 0]
            for a, b in zip(nz, nz[1:]):
                vox[a][-2:] = (1, 2, 3)
                vox[b][:2] = (1, 2, 3)
        c[name] = dict(name=name, fact=fact, clouds=[_cloud(rng, v, vs) for v in vox], vs=vs)
    add("block_edges", "frames of 256, 512 and 256 points: every boundary is a block boundary", [256, 512, 256])
    add("inside_run", "frames of 100, 37 and 300 points; one voxel's run straddles each boundary", [100, 37, 300], shared_run=True)
    add("empty_first", "an empty frame first", [0, 300, 45])
    add("empty_middle", "empty frames in the middle", [130, 0, 0, 77], shared_run=True)
    add("empty_last", "an empty frame last", [300, 45, 0])
    add("one_point", "one frame of one point", [1])
    add("max_frames", f"{MAX_FRAMES} frames of 37 points", [37] * MAX_FRAMES)
    return c


def compact_case(extra_voxel, vs=0.3):
    """N = 262 145 points (the smallest count with a compact table), R = max(N / 4, 65 536) = 65 536.  Two frames of a
    32^3 cube: frame 0 holds 32 768 voxels, frame 1 the same 32 768 -> 65 536 distinct rows, four points each in two runs
    of two, and one more point: a copy (exactly R voxels) or a voxel of its own (R + 1)."""
    n = COMPACT_ABOVE + 1
    R = compact_rows(n)
    assert R == 65536
    rng = np.random.default_rng(33)
    ids = np.arange(32 ** 3)
    cube = np.stack([ids % 32 - 16, (ids // 32) % 32 - 16, ids // 1024 - 16], 1)
    vox = []
    for b in range(2):
        order = rng.permutation(len(cube))
        vox.append(np.concatenate([np.repeat(cube[order], 2, axis=0), np.repeat(cube[order[::-1]], 2, axis=0)]))
    vox[1] = np.concatenate([vox[1], [[40, 40, 40]] if extra_voxel else vox[1][:1]])
    assert sum(len(v) for v in vox) == n
    return dict(name="compact_R_plus_1" if extra_voxel else "compact_R", fact=f"{R + int(extra_voxel)} distinct voxels for R = {R}",
                clouds=[_cloud(rng, v, vs) for v in vox], vs=vs, R=R, voxels=R + int(extra_voxel))


# ------------------------------------------------------------------------------------------------- fills and packs
FILL_PHASES = tuple(range(16))
FILL_LENGTHS = (0, 1, 3, 15, 16, 17, 40)
FILL_LONG = (FILL_8_PER_THREAD + 16 + 5, FILL_GRID_BYTES + 2048 * 256 * 16 + 16 + 7)      # (past 2048 * 256 * 16 bytes, past the capped grid)
FILL_GUARD = 64


def fill_head(phase):
    return (16 - phase) % 16


PACK_LONG_SOURCE = PACK_GRID_WORDS + 2 * 64 * 256 + 123       # three trips of the stride loop, the last one partial
PACK_LONG_ZERO = PACK_GRID_WORDS * 3 + 77
