"""Plain numpy restatements of the stand-alone graph primitives of csrc/graph.hip (ramp_group_by, ramp_group_by_small,
ramp_neighbors, ramp_neighbors_from_groups, ramp_segment_softmax_sum), and the seeded cases their tests share.  No torch.

The integer outputs are defined through np.lexsort with the edge index as the last key, so "stable" is spelled out and not
left to a sort's implementation.  The softmax works in float64 with the kernel's three passes."""
import zlib

import numpy as np

I64 = np.int64


# ------------------------------------------------------------------------------------------------------ references
def group_by(keys):
    """-> dict(order, gid, seg_start, ukeys, G): order = edges by (key, edge index); gid[e] = dense rank of keys[e] among the
    sorted distinct keys; seg_start[g] = first sorted position of group g, seg_start[G] = E; ukeys = the distinct keys"""
    keys = np.asarray(keys, I64)
    E = len(keys)
    order = np.lexsort((np.arange(E), keys)).astype(np.int32)
    ks = keys[order]
    head = np.ones(E, bool)
    head[1:] = ks[1:] != ks[:-1]
    pos = np.flatnonzero(head)
    gid = np.empty(E, np.int32)
    gid[order] = np.cumsum(head) - 1
    return dict(order=order, gid=gid, seg_start=np.append(pos, E).astype(np.int32), ukeys=ks[pos].astype(I64), G=len(pos))


def small_keys(a, b, mul, sub):
    """the key of ramp_group_by_small: a*mul + b - sub (b None: 0)"""
    a = np.asarray(a, I64)
    return a * I64(mul) + (0 if b is None else np.asarray(b, I64)) - I64(sub)


def neighbors(kk, jj):
    """-> (ix, jx, kj): kj = edges by (kk, jj, edge index); ix[e] / jx[e] = the edge before / after e in kj if it has e's kk,
    else -1"""
    kk, jj = np.asarray(kk, I64), np.asarray(jj, I64)
    E = len(kk)
    kj = np.lexsort((np.arange(E), jj, kk))
    ix, jx = np.full(E, -1, I64), np.full(E, -1, I64)
    if E > 1:
        same = kk[kj[1:]] == kk[kj[:-1]]
        ix[kj[1:][same]] = kj[:-1][same]
        jx[kj[:-1][same]] = kj[1:][same]
    return ix, jx, kj.astype(np.int32)


def segment_softmax_sum(fx, gx, gid, G):
    """-> (y, bound), float64 [G, C]: per group and channel m = max gx, s = sum exp(gx - m), y = sum (exp(gx - m) / s) fx in
    three passes, so that a column of -inf gives NaN (exp(-inf - -inf)) as torch_scatter's composite does;
    bound = sum (exp(gx - m) / s) |fx|, the scale of the rounding error of any evaluation of y"""
    fx, gx, gid = np.asarray(fx, np.float64), np.asarray(gx, np.float64), np.asarray(gid)
    C = fx.shape[1]
    y, bound = np.zeros((G, C)), np.zeros((G, C))
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            rows = np.flatnonzero(gid == g)
            m = gx[rows].max(0)
            w = np.exp(gx[rows] - m)
            w = w / w.sum(0)
            y[g] = (w * fx[rows]).sum(0)
            bound[g] = (w * np.abs(fx[rows])).sum(0)
    return y, bound


def softmax_tolerance(n, bound, ref=None, half=False):
    """per element: (n + 16) 2^-23 bound [+ 2^-11 |ref| for the one rounding of an fp16 output].  Each of the two n-term fp32
    sums rounds at most n times at 2^-24, expf and the division add a few ulps; the factor 2 is margin.  n: the group's size,
    broadcast against bound"""
    tol = (np.asarray(n, np.float64) + 16) * 2.0 ** -23 * bound
    return tol + 2.0 ** -11 * np.abs(ref) if half else tol


# ------------------------------------------------------------------------------------------------------ cases
E_EDGES = (0, 1, 2, 255, 256, 257, 4099)        # empty, one, a pair, around the 256-lane launch tail, 17 workgroups
SMALL_K = (1, 255, 1024, 1025, 4096, 4097, 10000)   # per = 1 | 2 in the scan at 1024 | 1025; LDS | global histogram at 4096 | 4097
NB_GROUP_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 3000)   # the 64-lane stride and the 1024-entry staging of the rank kernel
SOFTMAX_C = (1, 127, 128, 129, 384)
SOFTMAX_GROUP_SIZES = (1, 2, 17, 1000)
LONG_SEGMENT = 3000


def _rng(*seed):
    return np.random.default_rng([zlib.crc32(s.encode()) if isinstance(s, str) else int(s) for s in seed])


def keys_for_group_by(kind, E, seed=0):
    """-> (keys, bounds): the key set ``kind`` on E edges and the key_bound settings that are legal for it"""
    rng = _rng(1, E, seed)
    if kind == "random":
        keys = rng.integers(0, max(E // 4, 3), E).astype(I64)
    elif kind == "equal":
        keys = np.full(E, 5, I64)
    elif kind == "zeros":
        return np.zeros(E, I64), (0, 1)
    elif kind == "descending":
        keys = np.arange(E, 0, -1, dtype=I64) * 3
    elif kind == "pow2":                       # max + 1 is a power of two: the bound needs every one of its bits
        keys = rng.integers(0, 256, E).astype(I64)
        if E:
            keys[E // 2] = 255
    elif kind == "huge":                       # around 2^62: bit 62 decides, only bound 0 sorts it
        keys = (I64(1) << I64(62)) + rng.integers(-3, 3, E).astype(I64)
        return keys, (0,)
    else:
        raise KeyError(kind)
    top = int(keys.max()) + 1 if E else 1
    return keys, (0, top)


GROUP_BY_KINDS = ("random", "equal", "zeros", "descending", "pow2", "huge")


def neighbor_graph(kind, E, seed=0):
    """-> (kk, jj, settings): settings = the legal (kk_bound, jj_bound) pairs, covering (0, 0), the one composite pass (both
    given, bits summing to at most 62), the two passes with bounded bits (both given, sum above 62) and one bound alone"""
    rng = _rng(2, E, seed)
    if kind == "ties":                         # few kk, fewer jj: most of a group shares its jj, the edge index decides
        kk, jj = rng.integers(0, max(E // 40, 2), E), rng.integers(0, 3, E)
    elif kind == "single":
        kk, jj = np.full(E, 7), rng.integers(0, 5, E)
    elif kind == "distinct":
        kk, jj = rng.permutation(E), rng.integers(0, 5, E)
    else:
        raise KeyError(kind)
    kk, jj = kk.astype(I64), jj.astype(I64)
    kb, jb = (int(kk.max()) + 1, int(jj.max()) + 1) if E else (1, 1)
    return kk, jj, ((0, 0), (kb, jb), (1 << 40, 1 << 30), (kb, 0), (0, jb))


NEIGHBOR_KINDS = ("ties", "single", "distinct")


def small_case(kind, K, E, seed=0):
    """-> keys in [0, K) on E edges: "dense" (every value likely), "three" (three present keys out of K), "ends" (0 and K-1
    only)"""
    rng = _rng(3, K, E, seed)
    if kind == "dense":
        return rng.integers(0, K, E).astype(I64)
    if kind == "three":
        present = np.unique(np.array([K // 3, K // 2, K - 1], I64))
        return present[rng.integers(0, len(present), E)]
    if kind == "ends":
        return np.where(rng.integers(0, 2, E) == 1, K - 1, 0).astype(I64)
    raise KeyError(kind)


SMALL_KINDS = ("dense", "three", "ends")


def long_segment_case(K, seed=0):
    """one key with LONG_SEGMENT edges among 300 edges of other keys, shuffled: the rank sort's 64 lanes pass 47 times"""
    rng = _rng(4, K, seed)
    big = K // 2
    other = rng.integers(0, K, 300).astype(I64)
    other[other == big] = (big + 1) % K
    keys = np.concatenate([np.full(LONG_SEGMENT, big, I64), other])
    return keys[rng.permutation(len(keys))]


def pair_case(W, E, f_lo, seed=0):
    """-> (a, b, mul, sub, K): frame pairs in [f_lo, f_lo + W)^2, keyed as ramp_group_by_small's pair form"""
    rng = _rng(5, W, E, seed)
    a = (rng.integers(0, W, E) + f_lo).astype(I64)
    b = (rng.integers(0, W, E) + f_lo).astype(I64)
    return a, b, W, f_lo * W + f_lo, W * W


def bad_key_cases(K, seed=0):
    """-> [(name, a, b, mul, sub, K)]: 300 edges, every key in [0, K) but the one the name tells.  The pair form has
    W = isqrt(K) and its own K = W W (4096 -> 4096, 10000 -> 10000: one on either histogram path)"""
    rng = _rng(6, K, seed)
    E = 300
    base = rng.integers(0, K, E).astype(I64)
    minus, at_k = base.copy(), base.copy()
    minus[E // 3] = -1
    at_k[2 * E // 3] = K
    # the pair form with frames in [5, 5 + W): the right sub is 5 W + 5.  With sub = 5 W every key comes out 5 too large, which
    # stays inside [0, W W) for a < 5 + W - 1; the one planted edge (5 + W - 1, 5 + W - 2), in range under the right sub,
    # lands on W W + 3
    W = max(int(np.sqrt(K)), 6)
    a = (rng.integers(0, W - 1, E) + 5).astype(I64)
    b = (rng.integers(0, W, E) + 5).astype(I64)
    a[E // 2], b[E // 2] = 5 + W - 1, 5 + W - 2
    return [("minus_one", minus, None, 1, 0, K), ("at_K", at_k, None, 1, 0, K), ("wrong_sub", a, b, W, 5 * W, W * W)]


def sized_groups(sizes, seed=0, spread=3, n_jj=7):
    """-> (kk, jj): one kk per entry of ``sizes`` (ids ``spread`` apart, so absent keys lie between them), shuffled over the
    edges; jj from ``n_jj`` values, so a group of more than n_jj edges has ties"""
    rng = _rng(7, len(sizes), seed)
    kk = np.concatenate([np.full(n, 2 + spread * g, I64) for g, n in enumerate(sizes)])
    kk = kk[rng.permutation(len(kk))]
    return kk, rng.integers(0, n_jj, len(kk)).astype(I64)


def group_sizes(keys):
    return np.unique(np.asarray(keys), return_counts=True)[1]


def tracker_graph(scene, heavy=None):
    """(ii, jj, kk) of a scenes.ba_scene graph; heavy = (patch, count): that patch gets ``count`` factors in all, the extra
    ones to target frames drawn from the window (repeats of (kk, jj), so the edge index decides among them)"""
    ii, jj, kk = (np.asarray(scene[k], I64) for k in ("ii", "jj", "kk"))
    if heavy is not None:
        patch, count = heavy
        rng = _rng(8, patch, count)
        extra = count - int((kk == patch).sum())
        ii = np.concatenate([ii, np.full(extra, patch // scene["M"], I64)])
        jj = np.concatenate([jj, rng.integers(0, scene["n_frames"], extra).astype(I64)])
        kk = np.concatenate([kk, np.full(extra, patch, I64)])
        perm = rng.permutation(len(kk))
        ii, jj, kk = ii[perm], jj[perm], kk[perm]
    return ii, jj, kk


def softmax_case(C, kind, half=False, seed=0):
    """-> (fx, gx, keys) float32 / int64 with groups of SOFTMAX_GROUP_SIZES interleaved; values already rounded to fp16 when
    ``half``.  kind: "normal", "equal" (one gx per group), "peak" (+-big, one row at +big per group and channel),
    "some_inf" (-inf in about a third of the rows, never in all rows of a column), "all_inf" (as some_inf, and every row
    of the group of 17 is -inf in the even channels)"""
    rng = _rng(9, C, kind, int(half), seed)
    keys = np.concatenate([np.full(n, 10 + 4 * g, I64) for g, n in enumerate(SOFTMAX_GROUP_SIZES)])
    keys = keys[rng.permutation(len(keys))]
    E = len(keys)
    fx = rng.normal(size=(E, C)).astype(np.float32)
    gx = (3 * rng.normal(size=(E, C))).astype(np.float32)
    big = 65504.0 if half else 80.0
    if kind == "equal":
        gx[:] = (keys % 5 - 2)[:, None].astype(np.float32)
    elif kind == "peak":
        gx[:] = -big
        for k in np.unique(keys):
            rows = np.flatnonzero(keys == k)
            gx[rows[rng.integers(0, len(rows), C)], np.arange(C)] = big
    elif kind in ("some_inf", "all_inf"):
        hole = rng.random((E, C)) < 0.33
        for k in np.unique(keys):                      # one finite row per group and channel stays
            rows = np.flatnonzero(keys == k)
            hole[rows[rng.integers(0, len(rows), C)], np.arange(C)] = False
        gx[hole] = -np.inf
        if kind == "all_inf":
            gx[np.ix_(np.flatnonzero(keys == 10 + 4 * 2), np.arange(0, C, 2))] = -np.inf
    elif kind != "normal":
        raise KeyError(kind)
    if half:
        fx, gx = fx.astype(np.float16).astype(np.float32), gx.astype(np.float16).astype(np.float32)
    return fx, gx, keys


SOFTMAX_KINDS = ("normal", "equal", "peak", "some_inf", "all_inf")
