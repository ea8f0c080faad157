"""The device-side keyframe edit (csrc/track.hip trk_flag / trk_decide / trk_apply) and the graph plan behind it
(csrc/graph.hip plan_hist / plan_scan / plan_scatter / plan_segsort) against the numpy restatement tests/editref.py, at the
sizes, window boundaries, row counts, decisions and capacity limits of editref.CASES, and over chains of six edits.

Every comparison is exact.  Each step is ``DeviceTrack.step(counter, KEYFRAME | MM_GIVEN, E_bound)`` on a hand-filled graph,
``dyn``, ``mm`` and recognisable per-frame buffers.  The factor list's two halves are the test's own allocations (4 E_cap words
and a guard behind them, filled with a canary), the plan's outputs, the delta log and the edit scratch start from a canary
too: what a step has to write is compared, everything else has to keep its canary.  ``keyframe_index``, ``log_cap`` and
``n_rows`` are varied in the descriptor (the latter two only downwards, so the allocations exceed what the kernels are told).

A clean status word is asserted wherever tests/test_editref_cpu.py shows the case inside the device's capacities."""
import gc

import numpy as np
import pytest
import torch

import editref as er

pytestmark = pytest.mark.gpu

C64, C32, CF = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B, -7.5
FRAME_BUFS = (("tstamps_", 0), ("colors_", 0), ("poses_", 0), ("patches_", 0), ("intrinsics_", 0),
              ("imap_", er.MEM), ("gmap_", er.MEM), ("fmap1_", er.MEM), ("fmap2_", er.MEM))
_rigs = {}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


class Rig:
    """one tracker and its DeviceTrack per geometry, with test-owned factor lists"""

    def __init__(self, g):
        from rampvo_amd import ops, track_dev as td
        from rampvo_amd.config import make_cfg
        from rampvo_amd.Ramp_vo import Ramp_vo
        from rampvo_amd.synthetic import make_network
        self.g, self.td = g, td
        cfg = make_cfg(g.preset, PATCHES_PER_FRAME=g.M, MIXED_PRECISION=True)
        assert (cfg.PATCH_LIFETIME, cfg.REMOVAL_WINDOW, cfg.KEYFRAME_THRESH) == (g.r, g.R, er.THRESH)
        self.slam = slam = Ramp_vo(cfg, make_network("SingleScale"), {"event_bias": True}, ht=128, wd=192)
        self.dv = dv = td.DeviceTrack(slam)
        assert (dv.E_cap, dv.kk_cap, dv.ij_cap, dv.kkey_cap, dv.pkey_cap, dv.new_cap, slam.mem) == \
            (g.E_cap, g.kk_cap, g.ij_cap, g.kkey_cap, g.pkey_cap, g.new_cap, er.MEM)
        self.n_rows, self.log_cap = int(dv.t.n_rows), int(dv.t.log_cap)
        self.guard = g.new_cap + g.pad                       # one frame's factors and the defined rows behind them
        self.gbuf = [torch.full((4 * g.E_cap + self.guard,), C64, dtype=torch.int64, device="cuda") for _ in range(2)]
        for i in range(2):
            dv.graph[i] = self.gbuf[i][:4 * g.E_cap].view(4, g.E_cap)
            dv.t.graph[i] = self.gbuf[i].data_ptr()
        gen = torch.Generator(device="cuda").manual_seed(17)
        slam.tstamps_.copy_(torch.arange(100, 100 + slam.N, device="cuda"))
        xi = 0.2 * torch.randn((slam.N, 6), device="cuda", generator=gen)
        slam.poses_.copy_(ops.se3_unary("ramp_se3_exp", xi, 6, 7))
        for buf in (slam.patches_, slam.intrinsics_, slam.imap_, slam.gmap_, slam.fmap1_, slam.fmap2_):
            buf.copy_(torch.randn(buf.shape, device="cuda", generator=gen).to(buf.dtype))
        slam.colors_.copy_(torch.randint(0, 255, slam.colors_.shape, device="cuda", generator=gen).to(torch.uint8))
        self.pristine = {name: getattr(slam, name).clone() for name, _ in FRAME_BUFS}
        self.plan_out = [dv.kk[k] for k in ("order", "gid", "seg", "ngroups", "ukeys")] + \
                        [dv.ij[k] for k in ("order", "gid", "seg", "ngroups", "ukeys")] + [dv.ix, dv.jx, dv.kj]
        dv.active, dv._frames = True, 0

    # ------------------------------------------------------------------ state before a step
    def fresh(self, ii, jj, kk, n, status=0, nlog=0):
        """a hand-filled state: graph half 0 holds the factors, everything a step may write holds a canary"""
        dv, td, g = self.dv, self.td, self.g
        E = len(ii)
        for b in self.gbuf:
            b.fill_(C64)
        if E:
            dv.graph[0][:, :E] = _dev(np.stack([ii, jj, kk, np.arange(E, dtype=np.int64)]))
        dv.cur = 0
        d = np.zeros(td.DYN_WORDS, np.int32)
        flo = int(min(ii.min(), jj.min())) if E else 0
        d[td.DYN_N], d[td.DYN_NROW], d[td.DYN_E] = n, n - 1, E
        d[td.DYN_KLO], d[td.DYN_FLO], d[td.DYN_W] = (int(kk.min()) // g.M * g.M if E else 0), flo, n - flo
        d[td.DYN_STATUS], d[td.DYN_NLOG] = status, nlog
        dv.dyn.copy_(_dev(d))
        for name, _ in FRAME_BUFS:
            getattr(self.slam, name).copy_(self.pristine[name])
        self.state = dict(self.pristine)                     # expected logical rows (never written in place)
        dv.fmap1_slot.copy_(torch.arange(er.MEM, dtype=torch.int32, device="cuda"))
        dv.dlog.fill_(CF)
        dv.plan_ws.zero_()                                   # (the histograms start zeroed, as DeviceTrack allocates them)

    def step(self, n, KI, mm, counter, exp, E_bound=None, log_cap=None, n_rows=None, status=0, nlog=0, compare_plan=True,
             oversize=False):
        """one edit on graph half dv.cur and every check of it.  exp: editref.edit's result for this step (with "remove");
        status: the word expected afterwards"""
        dv, td, g, slam = self.dv, self.td, self.g, self.slam
        cur, E = dv.cur, int(exp["dyn"]["EPREV"])
        E_bound = max(E, 1) if E_bound is None else E_bound
        self.gbuf[1 - cur].fill_(C64)
        for t in self.plan_out:
            t.fill_(C64 if t.dtype == torch.int64 else C32)
        dv.edit_ws.fill_(C32)
        gin = self.gbuf[cur].clone()
        dlog_before = dv.dlog.clone()
        tab_before = dv.fmap1_slot.clone()
        dv.mm.copy_(torch.tensor(mm, dtype=torch.float32, device="cuda"))
        dv.t.keyframe_index = KI
        dv.t.log_cap = self.log_cap if log_cap is None else log_cap
        dv.t.n_rows = self.n_rows if n_rows is None else n_rows
        assert dv.t.log_cap <= self.log_cap and dv.t.n_rows <= self.n_rows and KI >= 2 and n >= KI + 1
        try:
            dv.step(counter=counter, flags=td.KEYFRAME | td.MM_GIVEN, E_bound=E_bound)
            torch.cuda.synchronize()
        finally:
            dv.t.log_cap, dv.t.n_rows = self.log_cap, self.n_rows
        out = 1 - cur
        # ---- sizes
        dd = dv.dyn.cpu().numpy()
        got_dyn = {name: int(dd[getattr(td, "DYN_" + name)]) for name in er.DYN}
        print("dyn", got_dyn, "status", int(dd[td.DYN_STATUS]), "expected", exp["dyn"], status)
        assert got_dyn == exp["dyn"]
        assert int(dd[td.DYN_FRAME]) == int(dd[td.DYN_FRAME2]) == counter
        assert int(dd[td.DYN_STATUS]) == status
        remove, k = exp["remove"], n - KI
        # ---- the factor list: kept ++ new, defined pad rows, canaries
        En, Ecap = exp["dyn"]["E"], g.E_cap
        got = dv.graph[out]
        assert torch.equal(got[:, :En], _dev(exp["graph"]))
        pad_end = min(En + g.pad, Ecap)
        pad_row = torch.tensor([0, 0, 0, -1], dtype=torch.int64, device="cuda")[:, None]
        assert (got[:, En:pad_end] == pad_row).all()
        assert (got[:, pad_end:] == C64).all() and (self.gbuf[out][4 * Ecap:] == C64).all()
        assert torch.equal(self.gbuf[cur], gin)
        # ---- delta log
        log_exp = dlog_before.clone()
        wrote = remove and nlog < int(dv.t.log_cap if log_cap is None else log_cap)
        assert int(dd[td.DYN_NLOG]) == nlog + int(wrote)
        if wrote:
            from rampvo_amd.lietorch import SE3
            poses = self.state["poses_"]
            ts = self.state["tstamps_"]
            log_exp[nlog, :2] = torch.stack([ts[k], ts[k - 1]]).to(torch.int32).view(torch.float32)
            log_exp[nlog, 2:9] = (SE3(poses[k]) * SE3(poses[k - 1]).inv()).data
        assert torch.equal(dv.dlog.view(torch.int32), log_exp.view(torch.int32))
        # ---- per-frame rows
        tab = dv.fmap1_slot.long()
        assert sorted(tab.tolist()) == list(range(er.MEM))
        if not remove:
            assert torch.equal(dv.fmap1_slot, tab_before)
        for name, ring in FRAME_BUFS:
            now = getattr(slam, name)
            if not remove:
                assert torch.equal(now[tab] if name == "fmap1_" else now, self.state[name]), name
                continue
            want = self.state[name][_dev(er.shift_source(k, n, now.shape[0], ring))]
            if name == "fmap1_":
                # the level-0 planes move by slot table; the freed slot goes to row n - 1 (the next frame's: content unspecified)
                now = now[tab]
                free = (n - 1) % ring
                want = want.clone()
                want[free] = now[free]
            assert torch.equal(now, want), name
            self.state[name] = want
        # ---- the plan of the new graph
        if not compare_plan:
            return dd
        fill = g.fill_bound(E_bound)
        assert En <= fill
        pl = er.plan(exp["graph"][0], exp["graph"][1], exp["graph"][2], exp["dyn"]["W"])
        ok_e = torch.ones(En, dtype=torch.bool, device="cuda")
        ok_pos = ok_e.clone()
        if oversize:
            sizes = np.diff(pl["kk"]["seg_start"])
            big = int(np.argmax(sizes))
            assert sizes[big] > er.PATCH_FACTORS_MAX and (sizes > er.PATCH_FACTORS_MAX).sum() == 1
            ok_e = _dev(pl["kk"]["gid"] != big)
            ok_pos[int(pl["kk"]["seg_start"][big]):int(pl["kk"]["seg_start"][big + 1])] = False
        for mine, ref in ((dv.kk, pl["kk"]), (dv.ij, pl["ij"])):
            ng = ref["ngroups"]
            assert int(mine["ngroups"].item()) == ng
            assert torch.equal(mine["order"][:En], _dev(ref["order"], torch.int32)) and (mine["order"][En:] == C32).all()
            assert torch.equal(mine["gid"][:En], _dev(ref["gid"], torch.int32))
            assert (mine["gid"][En:fill] == 0).all() and (mine["gid"][fill:] == C32).all()
            assert torch.equal(mine["seg"][:ng + 1], _dev(ref["seg_start"], torch.int32)) and (mine["seg"][ng + 1:] == C32).all()
            assert torch.equal(mine["ukeys"][:ng], _dev(ref["ukeys"])) and (mine["ukeys"][ng:] == C64).all()
        for mine, ref in ((dv.ix, pl["ix"]), (dv.jx, pl["jx"])):
            assert torch.equal(mine[:En][ok_e], _dev(ref)[ok_e])
            assert (mine[En:fill] == -1).all() and (mine[fill:] == C64).all()
        assert torch.equal(dv.kj[:En][ok_pos], _dev(pl["kj"], torch.int32)[ok_pos]) and (dv.kj[En:] == C32).all()
        return dd

    def add_frame(self, row, gen):
        """the per-frame rows a new frame stores at `row` (ring buffers modulo their length, level-0 planes by slot)"""
        slam, tab = self.slam, self.dv.fmap1_slot.long()
        for name, ring in FRAME_BUFS:
            buf = getattr(slam, name)
            at = row % ring if ring else row
            if name == "tstamps_":
                val = torch.tensor(5000 + row, device="cuda")
            elif name == "colors_":
                val = torch.randint(0, 255, buf.shape[1:], device="cuda", generator=gen).to(torch.uint8)
            elif name == "poses_":
                q = torch.randn(4, device="cuda", generator=gen)
                val = torch.cat([torch.randn(3, device="cuda", generator=gen), q / q.norm()])
            else:
                val = torch.randn(buf.shape[1:], device="cuda", generator=gen).to(buf.dtype)
            buf[int(tab[at]) if name == "fmap1_" else at] = val
            self.state[name] = self.state[name].clone()
            self.state[name][at] = val


def _rig(name):
    if name not in _rigs:
        _rigs[name] = Rig(er.GEOMS[name])
    return _rigs[name]


@pytest.fixture(scope="module", autouse=True)
def _drop_rigs():
    yield
    _rigs.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run_case(c, counter, status_in=0):
    rig = _rig(c.geom)
    ii, jj, kk = er.case_graph(c)
    exp = er.case_expected(c, (ii, jj, kk))
    rig.fresh(ii, jj, kk, c.n, status=status_in, nlog=c.nlog)
    return rig.step(c.n, c.KI, c.mm, counter, exp, E_bound=c.E_bound, log_cap=c.log_cap, n_rows=c.n_rows,
                    status=status_in | c.flag, nlog=c.nlog, compare_plan=c.flag != er.ST_BOUND, oversize=c.mode == "oversize")


@torch.no_grad()
@pytest.mark.parametrize("cid", [c.id for c in er.CASES if not c.flag])
def test_edit_and_plan_match_the_numpy_restatement(cid):
    """sizes, window boundaries, row shifts and decisions of editref.CASES: dyn, the factor list with its row column and pad
    rows, the log entry, every per-frame buffer and the whole plan, exact; status 0"""
    c = next(c for c in er.CASES if c.id == cid)
    if "decide" in c.id:
        assert er.decide(c.mm, er.THRESH) == {tag: dropped for tag, _, dropped in er.DECISIONS}[c.id[len("A-decide-"):]]
    _run_case(c, counter=77 + er.CASE_IDS.index(cid))


@torch.no_grad()
@pytest.mark.parametrize("cid", [c.id for c in er.CASES if c.flag])
def test_capacity_limits_set_their_status_bit_and_stay_in_bounds(cid):
    """factor capacity (4), an oversized patch (8), a full delta log (16), a launch bound below the live count (32), full
    frame buffers (64): the bit, the clamped sizes, everything still written exactly and nothing outside -- and the bit
    stays set through a clean step"""
    c = next(c for c in er.CASES if c.id == cid)
    dd = _run_case(c, counter=300)
    assert int(dd[_rig(c.geom).td.DYN_STATUS]) == c.flag
    clean = next(x for x in er.CASES if x.id == "A-size-1025-drop")
    dd = _run_case(clean, counter=301, status_in=c.flag)
    assert int(dd[_rig(c.geom).td.DYN_STATUS]) == c.flag


@torch.no_grad()
@pytest.mark.parametrize("geom", sorted(er.CHAINS))
def test_six_edits_in_a_row(geom):
    """(keep, drop, drop, keep, drop, keep) on alternating halves of the factor list, the numpy restatement carried along:
    each plan starts from the histograms the previous one cleared, each edit keeps the factors the previous one added
    (row -1) under their own index"""
    rig = _rig(geom)
    gen = torch.Generator(device="cuda").manual_seed(23)
    for s in er.chain_steps(geom):
        ii, jj, kk = s["graph"]
        if s["step"] == 0:
            rig.fresh(ii, jj, kk, s["n"])
            rig.state = {name: t.clone() for name, t in rig.state.items()}
        exp = dict(s["out"], remove=s["remove"])
        nlog = sum(er.CHAIN_PATTERN[:s["step"]])
        rig.step(s["n"], 4, s["mm"], 500 + s["step"], exp, status=0, nlog=nlog)
        assert rig.dv.cur == (s["step"] + 1) % 2
        rig.add_frame(exp["dyn"]["NROW"], gen)


def test_edit_scratch_covers_the_edit_workgroups():
    """edit_ws holds three words per edit workgroup of editref.EDIT_BLOCK (csrc/track.hip TRK_EB) factors"""
    dv = _rig("A").dv
    assert dv.edit_ws.numel() >= 3 * -(-dv.E_cap // er.EDIT_BLOCK)
