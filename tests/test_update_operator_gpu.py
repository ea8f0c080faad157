"""ramp_update_forward (csrc/update_op.hip: the update operator's launch sequence, shared by the device-resident step and
FusedUpdate.hidden) against the same operator chained here from the per-stage exports -- bit for bit: the entry adds no
arithmetic, it only orders launches.  Weights: make_network("SingleScale"); inputs seeded; the group tables and temporal
neighbours are GraphPlan.build's on a random graph; the state comes through a row map with -1 entries, the context through
an index with a modulus."""
import ctypes

import pytest
import torch

from rampvo_amd._lib import RAMP_EINVAL

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1003]          # one row, both sides of the 64-row tile, a ragged tail
WD, HT = 40.0, 30.0


@pytest.fixture(scope="module")
def fused():
    """{fp32 flag: (FusedUpdate, its weights)} on the default paths"""
    from rampvo_amd.synthetic import make_network
    out = {}
    for x3, T in ((0, torch.float16), (1, torch.float32)):
        fu = make_network("SingleScale").update.fused(T)
        assert fu.use_x3 == bool(x3) and fu.use_mlp
        out[x3] = (fu, fu.weights())
    return out


_cases = {}


def _case(E, x3):
    """seeded operands of one call (shared by the tests, never written)"""
    if (E, x3) in _cases:
        return _cases[(E, x3)]
    from rampvo_amd.net import GraphPlan
    T = torch.float32 if x3 else torch.float16
    g = torch.Generator().manual_seed(100 + E)
    M = 40
    kk = torch.sort(torch.randint(0, M * 6, (E,), generator=g)).values.cuda()
    c = dict(E=E, T=T, plan=GraphPlan.build(kk // M, torch.randint(0, 8, (E,), generator=g).cuda(), kk))
    rows = max(7 * E // 10, 1)
    c["net"] = (torch.randn(rows, 384, generator=g) * 0.5).cuda()
    c["net_map"] = torch.randint(-1, rows, (E,), generator=g).cuda()
    c["net_map"][::3] = -1
    c["inp"] = (torch.randn(300, 384, generator=g) * 0.5).to(T).cuda()
    c["inp_idx"] = torch.randint(0, 5000, (E,), generator=g).cuda()
    c["corr"] = torch.nn.functional.pad((torch.randn(E, 882, generator=g) * 0.5).to(T), (0, 14)).contiguous().cuda()
    c["coords"] = (torch.rand(E, 2, 3, 3, generator=g) * 60).cuda()
    _cases[(E, x3)] = c
    return c


def _buffers(c, x3, heads, fill=None):
    """the scratch and output tensors of one ramp_update_forward call (fill: a canary value for all of them)"""
    from rampvo_amd._lib import lib
    E, T, p, dev = max(c["E"], 1), c["T"], c["plan"], "cuda"
    Gkk, Gij = max(p.max_kk, 1), max(p.max_ij, 1)
    new = lambda *s, dtype=torch.float32: (torch.empty(*s, dtype=dtype, device=dev) if fill is None
                                           else torch.full(s, fill, dtype=dtype, device=dev))
    b = dict(state0=new(E, 384), state1=new(E, 384), net_out=new(E, 384), hkk=new(Gkk, 384, dtype=T), hij=new(Gij, 384, dtype=T))
    if x3:
        b.update(fg=new(E, 768), ykk=new(Gkk, 384), yij=new(Gij, 384))
    else:
        b["sagg_frag"] = new(lib().ramp_upd_softagg_frag_rows(E, max(Gkk, Gij)), 3, 384)     # (a size query, no stage)
    if heads:
        b.update(target=new(1, E, 2), weight=new(1, E, 2))
    else:
        b["relu_out"] = new(E, 384, dtype=T)
    return b


def _args(fu, c, x3, heads, b, E=None):
    from rampvo_amd._lib import UpdateArgs
    p = c["plan"]
    a = UpdateArgs(E=c["E"] if E is None else E, kk_cap=max(p.max_kk, 1), ij_cap=max(p.max_ij, 1), inp_mod=300, fp32=x3, P=3,
                   wd=WD, ht=HT)
    a.w = ctypes.pointer(fu.record())
    t = dict(corr=c["corr"], net_prev=c["net"], net_map=c["net_map"], inp=c["inp"], inp_idx=c["inp_idx"],
             kk_order=p.g_kk.order, kk_gid=p.g_kk.gid, kk_seg=p.g_kk.seg_start, kk_ngroups=p.g_kk.ngroups,
             ij_order=p.g_ij.order, ij_gid=p.g_ij.gid, ij_seg=p.g_ij.seg_start, ij_ngroups=p.g_ij.ngroups, ix=p.ix_raw,
             jx=p.jx_raw, coords=c["coords"] if heads else None)
    t.update({k: v for k, v in b.items() if not k.startswith("state")})
    for name, ten in t.items():
        setattr(a, name, ten.data_ptr() if ten is not None else None)
    a.state[0], a.state[1] = b["state0"].data_ptr(), b["state1"].data_ptr()
    return a


def _forward(fu, c, x3, heads):
    from rampvo_amd._lib import check, lib, stream
    b = _buffers(c, x3, heads)
    check(lib().ramp_update_forward(ctypes.byref(_args(fu, c, x3, heads, b)), stream()), "ramp_update_forward")
    return (b["net_out"], b["target"], b["weight"]) if heads else (b["net_out"], b["relu_out"])


def _softagg_x3(fu, x32, add_t, add_idx, fg_pack, h_pack, groups, max_groups):
    """one fp32 SoftAgg from its three exports (fg, segment_softmax, linear); h's rows at and above the group count zero"""
    fg = fu.fg(x32, add_t, add_idx, fg_pack, x32.shape[0], write_back=False)
    return fu.h_lin(fu.seg(fg, groups, max(int(max_groups), 1)), h_pack, groups)


def _chained(fu, w, c, x3, heads, write_back=False):
    """the operator from the per-stage exports.  fp32: the step's form throughout (ramp_x3_gru takes both SoftAgg tables).
    fp16: the pair SoftAgg reads net + hkk[gid] without a write-back, as in the step; ramp_upd_gru takes ONE table, so the
    sum it starts from is written by ramp_upd_row_fuse -- write_back=True: before the pair SoftAgg already, which then adds
    nothing (the host-driven path's form before the two shared one sequence)"""
    from rampvo_amd._lib import check, lib, ptr, stream
    E, p = c["E"], c["plan"]
    s0 = fu.corr_mlp(c["corr"], c["net"], c["net_map"], c["inp"], c["inp_idx"], 300)
    s0 = fu.nbr(fu.nbr(s0, p.ix_raw, "c1"), p.jx_raw, "c2")
    heads_at = (c["coords"], WD, HT) if heads else None
    if x3:
        hkk = _softagg_x3(fu, s0, None, None, w["kk_fg_pack"], w["kk_h_pack"], p.g_kk, p.max_kk)
        hij = _softagg_x3(fu, s0, hkk, p.g_kk.gid, w["ij_fg_pack"], w["ij_h_pack"], p.g_ij, p.max_ij)
        return fu.gru(s0, add=(hij, p.g_ij.gid), add0=(hkk, p.g_kk.gid), heads_at=heads_at)
    hkk = fu.softagg(s0, None, None, w["kk_fg_pack"], w["kk_h_pack"], p.g_kk, p.max_kk, E)
    summed = torch.empty(E, 384, device="cuda")

    def write_sum():
        # (a direct call: a row kernel of the library-GEMM path, no stage of the fused chains)
        check(lib().ramp_upd_row_fuse(ptr(s0), None, ptr(hkk), None, None, ptr(p.g_kk.gid), 0, None, None, None, None, 0.0, 0,
                                      ptr(summed), None, E, 1, stream()), "ramp_upd_row_fuse")
    if write_back:
        write_sum()
        hij = fu.softagg(summed, None, None, w["ij_fg_pack"], w["ij_h_pack"], p.g_ij, p.max_ij, E)
    else:
        hij = fu.softagg(s0, hkk, p.g_kk.gid, w["ij_fg_pack"], w["ij_h_pack"], p.g_ij, p.max_ij, E)
        write_sum()
    return fu.gru(summed, add=(hij, p.g_ij.gid), heads_at=heads_at)


def _assert_equal(got, ref, what):
    for name, a, b in zip(("out32", "relu / target", "weight"), got, ref):
        assert torch.isfinite(b.float()).all(), (what, name)
        assert torch.equal(a, b), (what, name, float((a.float() - b.float()).abs().max()))


@pytest.mark.parametrize("heads", [False, True], ids=["relu", "heads"])
@pytest.mark.parametrize("x3", [0, 1], ids=["fp16", "fp32x3"])
@pytest.mark.parametrize("E", SIZES)
@torch.no_grad()
def test_update_forward_equals_the_chained_stages_bit_for_bit(fused, E, x3, heads):
    fu, w = fused[x3]
    c = _case(E, x3)
    _assert_equal(_forward(fu, c, x3, heads), _chained(fu, w, c, x3, heads), (E, x3, heads))


@pytest.mark.parametrize("heads", [False, True], ids=["relu", "heads"])
@pytest.mark.parametrize("E", SIZES)
@torch.no_grad()
def test_update_forward_equals_the_written_back_fp16_form(fused, E, heads):
    """the host-driven fp16 path used to write net + hkk[gid] back (ramp_upd_row_fuse) between the two SoftAggs, where the
    step lets the pair SoftAgg and the gru launch form the sum: the same fp32 additions in the same order"""
    fu, w = fused[0]
    c = _case(E, 0)
    _assert_equal(_forward(fu, c, 0, heads), _chained(fu, w, c, 0, heads, write_back=True), (E, heads))


@pytest.mark.parametrize("x3", [0, 1], ids=["fp16", "fp32x3"])
@torch.no_grad()
def test_update_forward_without_rows_and_with_missing_pointers_launches_nothing(fused, x3):
    """E = 0: RAMP_OK and every output / scratch tensor keeps its canary.  A required pointer nulled (each in turn, for the
    operands both precisions need and the precision's own SoftAgg workspace, with heads and without; one weight of the
    record too): RAMP_EINVAL, canaries intact again -- the check comes before the first launch"""
    from rampvo_amd._lib import TrackWeights, lib, stream
    fu, _ = fused[x3]
    c = _case(65, x3)
    canary = 1234.0                      # (exact in fp16)

    def untouched(b):
        torch.cuda.synchronize()
        return all(bool((t == canary).all()) for t in b.values())

    for heads in (False, True):
        b = _buffers(c, x3, heads, fill=canary)
        assert lib().ramp_update_forward(ctypes.byref(_args(fu, c, x3, heads, b, E=0)), stream()) == 0
        assert untouched(b)
        needed = ["w", "corr", "inp", "net_out", "kk_order", "kk_gid", "kk_seg", "kk_ngroups", "ij_order", "ij_gid", "ij_seg",
                  "ij_ngroups", "ix", "jx", "hkk", "hij"]
        needed += ["fg", "ykk", "yij"] if x3 else ["sagg_frag"]
        needed += ["target", "weight"] if heads else ["relu_out"]
        for name in needed + ["state0", "state1", "a weight"]:
            a = _args(fu, c, x3, heads, b)
            if name.startswith("state"):
                a.state[int(name[-1])] = None
            elif name == "a weight":
                rec = TrackWeights()
                ctypes.memmove(ctypes.byref(rec), ctypes.byref(fu.record()), ctypes.sizeof(rec))
                rec.ij_wh = None
                a.w = ctypes.pointer(rec)
            elif name == "w":
                a.w = ctypes.POINTER(TrackWeights)()
            else:
                setattr(a, name, None)
            assert lib().ramp_update_forward(ctypes.byref(a), stream()) == RAMP_EINVAL, name
        assert lib().ramp_update_forward(None, stream()) == RAMP_EINVAL
        assert untouched(b)
