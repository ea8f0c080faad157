"""Forward of the update operator (reference: ramp/net.py:69-90).

The hidden state stays fp32; the Linear layers' inputs / outputs are ``dtype`` (half under MIXED_PRECISION -- what the
reference's autocast does -- or float).  ``FusedUpdate.hidden`` is one C call on the fused GEMM chains (the device-resident
step's launch sequence, csrc/update_op.hip), or, as an A/B and test reference, library GEMMs stitched by the row kernels
of csrc/update.hip.  Weight copies in the formats both read are cached per module.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib, switches
from ._lib import TrackWeights, UpdateArgs, check, lib, ptr, stream

_code = {torch.float32: _lib.RAMP_F32, torch.float16: _lib.RAMP_F16}


CORR_ROW = 896     # correlation rows are padded from 882 to 896 elements on the GPU (zero tail)


def pack_linear_f16(weight):
    """nn.Linear weight [N, K] -> fp16 MFMA B fragments [K/32][N/16][64 lanes][8]:
    lane (q = lane >> 4, j = lane & 15) of fragment (ks, nt) holds W[16 nt + j][32 ks + 8 q .. + 8]"""
    w = weight.detach().half()
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0
    return w.view(N // 16, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous()


def pack_linear_x3(weight):
    """nn.Linear weight [N = 384, K] (K a multiple of 32) -> the split-fp16 pack of csrc/update_x3.hip: a flat fp16 tensor
    [K/32][N/16][2][64 lanes][8] -- plane 0 = fp16(W 2^s), plane 1 = fp16(W 2^s - plane 0), fragment order as
    pack_linear_f16 -- followed by the float 2^-s (as two fp16 slots) and padding to 16 bytes; s is the power of two that
    puts max |W| into [2^12, 2^13): the high part, the high part times 2^-11 and the low part are then fp16 NORMAL numbers"""
    import math
    w = weight.detach().float()
    N, K = w.shape
    assert N == 384 and K % 32 == 0
    amax = float(w.abs().max())
    s = 13 - math.frexp(amax)[1] if amax > 0 and math.isfinite(amax) else 0      # amax = m 2^e, m in [0.5, 1)
    ws = w * (2.0 ** s)                                    # exact
    hi = ws.half()
    lo = (ws - hi.float()).half()
    frag = lambda t: t.view(N // 16, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4)          # [K/32][N/16][4][16][8]
    planes = torch.stack([frag(hi), frag(lo)], dim=2).contiguous().view(-1)                 # [K/32][N/16][2][64][8]
    inv = torch.tensor([2.0 ** -s], dtype=torch.float32, device=w.device).view(torch.float16)
    return torch.cat([planes, inv, torch.zeros(6, dtype=torch.float16, device=w.device)]).contiguous()


class FusedUpdate:
    """Two paths.  The default one is a single C call, ``ramp_update_forward`` (csrc/update_op.hip): the launch sequence the
    device-resident step makes, on the fused chains of csrc/update_mlp.hip (fp16) / csrc/update_x3.hip (fp32).  The
    library-GEMM path -- ``use_mlp = False`` (fp16, tests) or RAMP_X3=0 (fp32, A/B runs) -- stitches hipBLASLt GEMMs with the
    row kernels of csrc/update.hip."""

    def __init__(self, update, dtype):
        self.m = update
        self.dtype = dtype
        self._w = self._key = self._rec = None
        self._params = list(update.parameters())     # module structure is fixed; values are tracked by key
        self._act_ok = True
        self.use_mlp = True
        self.use_x3 = dtype == torch.float32 and switches.read().x3
        self.last_tw = None                      # (target, weight) of the last hidden(..., heads_at=...) on the default path

    # ------------------------------------------------------------------ weights
    def weights(self):
        key = tuple([(p.data_ptr(), p._version) for p in self._params])
        if self._w is not None and key == self._key:
            return self._w
        m, T = self.m, self.dtype
        c = lambda t: t.detach().to(T).contiguous()
        f = lambda t: t.detach().float().contiguous()
        w = dict(
            corr0=(c(m.corr[0].weight), c(m.corr[0].bias)),
            corr0_pad=(c(F.pad(m.corr[0].weight, (0, CORR_ROW - m.corr[0].weight.shape[1]))), c(m.corr[0].bias)),
            corr2=(c(m.corr[2].weight), c(m.corr[2].bias)),
            corr_ln=(f(m.corr[3].weight), f(m.corr[3].bias), m.corr[3].eps),
            corr5=(c(m.corr[5].weight), c(m.corr[5].bias)),
            norm=(f(m.norm.weight), f(m.norm.bias), m.norm.eps),
            c1a=(c(m.c1[0].weight), c(m.c1[0].bias)), c1b=(c(m.c1[2].weight), c(m.c1[2].bias)),
            c2a=(c(m.c2[0].weight), c(m.c2[0].bias)), c2b=(c(m.c2[2].weight), c(m.c2[2].bias)),
            kk_fg=(c(torch.cat([m.agg_kk.f.weight, m.agg_kk.g.weight], 0)),
                   c(torch.cat([m.agg_kk.f.bias, m.agg_kk.g.bias], 0))),
            kk_h=(c(m.agg_kk.h.weight), c(m.agg_kk.h.bias)),
            ij_fg=(c(torch.cat([m.agg_ij.f.weight, m.agg_ij.g.weight], 0)),
                   c(torch.cat([m.agg_ij.f.bias, m.agg_ij.g.bias], 0))),
            ij_h=(c(m.agg_ij.h.weight), c(m.agg_ij.h.bias)),
            ln1=(f(m.gru[0].weight), f(m.gru[0].bias), m.gru[0].eps),
            g1_gate=(c(m.gru[1].gate[0].weight), c(m.gru[1].gate[0].bias)),
            g1_r1=(c(m.gru[1].res[0].weight), c(m.gru[1].res[0].bias)),
            g1_r2=(c(m.gru[1].res[2].weight), c(m.gru[1].res[2].bias)),
            ln2=(f(m.gru[2].weight), f(m.gru[2].bias), m.gru[2].eps),
            g2_gate=(c(m.gru[3].gate[0].weight), c(m.gru[3].gate[0].bias)),
            g2_r1=(c(m.gru[3].res[0].weight), c(m.gru[3].res[0].bias)),
            g2_r2=(c(m.gru[3].res[2].weight), c(m.gru[3].res[2].bias)),
            heads=(c(torch.cat([m.d[1].weight, m.w[1].weight], 0)), c(torch.cat([m.d[1].bias, m.w[1].bias], 0))),
        )
        self._rec = None
        if T == torch.float16 or self.use_x3:
            # the fused chains: weights in MFMA fragment order (fp16) / as split-fp16 packs (fp32); biases fp32 -- on the fp16
            # path the values of their fp16 roundings (they are half tensors under the reference's autocast)
            pack = pack_linear_x3 if self.use_x3 else pack_linear_f16
            px = lambda l, pad=0: (pack(F.pad(l.weight, (0, pad)) if pad else l.weight), f(c(l.bias)))
            gru = [px(l) for l in (m.gru[1].gate[0], m.gru[1].res[0], m.gru[1].res[2], m.gru[3].gate[0], m.gru[3].res[0],
                                   m.gru[3].res[2])]
            wp, bs = [g[0] for g in gru], [g[1] for g in gru]
            w["gru_pack"] = (wp, bs, (ctypes.c_void_p * 6)(*[t.data_ptr() for t in wp]),
                             (ctypes.c_void_p * 6)(*[t.data_ptr() for t in bs]))
            w["c1_pack"], w["c2_pack"] = px(m.c1[0]) + px(m.c1[2]), px(m.c2[0]) + px(m.c2[2])
            w["kk_fg_pack"], w["ij_fg_pack"] = px(m.agg_kk.f) + px(m.agg_kk.g), px(m.agg_ij.f) + px(m.agg_ij.g)
            w["kk_h_pack"], w["ij_h_pack"] = px(m.agg_kk.h), px(m.agg_ij.h)
            w["corr1_pack"] = px(m.corr[0], CORR_ROW - m.corr[0].weight.shape[1])
            w["tail_pack"] = px(m.corr[2]) + px(m.corr[5])
            w["heads_pack"] = (w["heads"][0], f(w["heads"][1]))
            self._rec = self._record(w)
        self._w, self._key = w, key
        return w

    @staticmethod
    def _record(w):
        """the packs as a ramp_track_weights record (the tensors stay alive in w)"""
        r = TrackWeights()
        P = lambda x: x.data_ptr()
        r.corr_w1, r.corr_b1 = map(P, w["corr1_pack"])
        r.corr_w2, r.corr_b2, r.corr_w3, r.corr_b3 = map(P, w["tail_pack"])
        r.c1_wa, r.c1_ba, r.c1_wb, r.c1_bb = map(P, w["c1_pack"])
        r.c2_wa, r.c2_ba, r.c2_wb, r.c2_bb = map(P, w["c2_pack"])
        r.kk_wf, r.kk_bf, r.kk_wg, r.kk_bg = map(P, w["kk_fg_pack"])
        r.ij_wf, r.ij_bf, r.ij_wg, r.ij_bg = map(P, w["ij_fg_pack"])
        r.kk_wh, r.kk_bh = map(P, w["kk_h_pack"])
        r.ij_wh, r.ij_bh = map(P, w["ij_h_pack"])
        for ln in ("corr_ln", "norm", "ln1", "ln2"):
            setattr(r, ln + "_w", P(w[ln][0]))
            setattr(r, ln + "_b", P(w[ln][1]))
            setattr(r, ln + "_eps", float(w[ln][2]))
        for i in range(6):
            r.gru_w[i], r.gru_b[i] = P(w["gru_pack"][0][i]), P(w["gru_pack"][1][i])
        r.heads_w, r.heads_b = map(P, w["heads_pack"])
        return r

    def record(self):
        """the ramp_track_weights record of the current weights: built once per weights key, read by ramp_update_forward
        and copied by DeviceTrack.bind_weights"""
        self.weights()
        if self._rec is None:
            raise RuntimeError("FusedUpdate: the library-GEMM path (RAMP_X3=0) has no fused-chain weights")
        return self._rec

    # ------------------------------------------------------------------ forward
    def hidden(self, net, inp_table, inp_idx, inp_mod, corr, plan, net_map=None, heads_at=None, net32_buf=None, out32_buf=None):
        """net [*,384] fp32 or None (zeros), row net_map[e] of it per edge when net_map is given (-1: zero
        row); inp = inp_table[inp_idx % inp_mod] (or inp_table rows when inp_idx is None); corr [E,896] (or dense [E,882]) in
        self.dtype.  Returns (net_out fp32 [E,384], relu copy in self.dtype).  heads_at = (coords [E,2,P,P], wd, ht), default
        path: the gru launch also forms the heads and target / weight (left in self.last_tw; the relu copy is then None).
        net32_buf / out32_buf: the library-GEMM path only (_hidden_gemm)."""
        self.last_tw = None
        x3 = self.use_x3
        if not (x3 or (self.dtype == torch.float16 and self.use_mlp)):
            return self._hidden_gemm(net, inp_table, inp_idx, inp_mod, corr, plan, net_map, net32_buf, out32_buf)
        E, dev, T, f32 = corr.shape[0], corr.device, self.dtype, torch.float32
        if corr.shape[1] != CORR_ROW:          # (a caller with dense [E, 882] rows: zero tail for the 16-byte row loads)
            corr = F.pad(corr, (0, CORR_ROW - corr.shape[1]))
        new = lambda *shape, dtype=f32, zero=False: (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=dev)
        g_kk, g_ij, Gkk, Gij = plan.g_kk, plan.g_ij, max(int(plan.max_kk), 1), max(int(plan.max_ij), 1)
        state = new(E, 384), new(E, 384)
        t = dict(corr=corr.contiguous(), net_prev=net, net_map=net_map, inp=inp_table.to(T), inp_idx=inp_idx,
                 net_out=state[1], kk_order=g_kk.order, kk_gid=g_kk.gid, kk_seg=g_kk.seg_start, kk_ngroups=g_kk.ngroups,
                 ij_order=g_ij.order, ij_gid=g_ij.gid, ij_seg=g_ij.seg_start, ij_ngroups=g_ij.ngroups, ix=plan.ix_raw,
                 jx=plan.jx_raw,
                 # the SoftAgg tables h(y); fp32: the h launch writes the rows below the group count only
                 hkk=new(Gkk, 384, dtype=T, zero=x3), hij=new(Gij, 384, dtype=T, zero=x3))
        if x3:
            t.update(fg=new(E, 768), ykk=new(Gkk, 384), yij=new(Gij, 384))
        else:
            t["sagg_frag"] = new(lib().ramp_upd_softagg_frag_rows(E, max(Gkk, Gij)), 3, 384)
        a = UpdateArgs(E=E, kk_cap=Gkk, ij_cap=Gij, inp_mod=int(inp_mod or 0), fp32=int(x3), P=3)
        if heads_at is not None:
            coords, wd, ht = heads_at
            a.P, a.wd, a.ht = coords.shape[-1], float(wd), float(ht)
            t.update(coords=coords, target=new(1, E, 2), weight=new(1, E, 2))
            self.last_tw = (t["target"], t["weight"])
        else:
            t["relu_out"] = new(E, 384, dtype=T)
        a.w = ctypes.pointer(self.record())
        a.state[0], a.state[1] = state[0].data_ptr(), state[1].data_ptr()
        for name, ten in t.items():
            setattr(a, name, ten.data_ptr() if ten is not None else None)
        check(lib().ramp_update_forward(ctypes.byref(a), stream()), "ramp_update_forward")
        return state[1], t.get("relu_out")

    # --------------------------------------------------------------- the library-GEMM path
    def lin(self, x, wb):
        return F.linear(x, wb[0], wb[1])

    def lin_relu(self, x, wb):
        if self._act_ok:
            try:
                return torch._addmm_activation(wb[1], x, wb[0].t(), use_gelu=False)
            except Exception:
                self._act_ok = False
        return F.relu_(F.linear(x, wb[0], wb[1]))

    def row_fuse(self, E, A=None, B=None, C=None, idxB=None, idxB32=None, modB=0, idxC32=None, ln=None, relu=False,
                 want_f32=False, want_t=False, out_f32=None, idxA=None):
        dev = (A if A is not None else B).device
        if want_f32 and out_f32 is None:
            out_f32 = torch.empty(E, 384, dtype=torch.float32, device=dev)
        out_t = torch.empty(E, 384, dtype=self.dtype, device=dev) if want_t else None
        check(lib().ramp_upd_row_fuse(ptr(A), ptr(idxA), ptr(B), ptr(C), ptr(idxB), ptr(idxB32), int(modB), None,
                                      ptr(idxC32),
                                      ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None,
                                      float(ln[2]) if ln else 0.0, int(relu), ptr(out_f32), ptr(out_t), E,
                                      _code[self.dtype], stream()), "ramp_upd_row_fuse")
        return out_f32, out_t

    def gather_mask(self, X, idx, E):
        out = torch.empty(E, 384, dtype=self.dtype, device=X.device)
        check(lib().ramp_upd_gather_mask(ptr(X), ptr(idx), ptr(out), E, _code[self.dtype], stream()),
              "ramp_upd_gather_mask")
        return out

    def gated(self, X, G, R, E, ln=None, want_f32=True, want_t=False, want_relu=False, out=None):
        dev = X.device
        o32 = (out if out is not None else torch.empty(E, 384, dtype=torch.float32, device=dev)) if want_f32 else None
        ot = torch.empty(E, 384, dtype=self.dtype, device=dev) if want_t else None
        orl = torch.empty(E, 384, dtype=self.dtype, device=dev) if want_relu else None
        check(lib().ramp_upd_gated(ptr(X), ptr(G), ptr(R), ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None,
                                   float(ln[2]) if ln else 0.0, ptr(o32), ptr(ot), ptr(orl), E, _code[self.dtype],
                                   stream()), "ramp_upd_gated")
        return o32, ot, orl

    def seg(self, fg, groups, max_groups):
        y = torch.empty(max(max_groups, 1), 384, dtype=self.dtype, device=fg.device)     # the kernel writes every row
        grp = (ptr(groups.order), ptr(groups.seg_start), ptr(groups.ngroups))
        if self.use_x3:
            check(lib().ramp_x3_segment_softmax(ptr(fg), *grp, ptr(y), int(max_groups), stream()), "ramp_x3_segment_softmax")
        else:
            check(lib().ramp_upd_segment_softmax(ptr(fg), *grp, ptr(y), int(max_groups), _code[self.dtype], stream()),
                  "ramp_upd_segment_softmax")
        return y

    # ------------------------------------------------------------------ single stages of the fused chains
    # One wrapper per exported stage, on the module's own packs (fg, softagg and h_lin are handed theirs, as they always were):
    # ramp_upd_* (fp16 features) or ramp_x3_* (fp32 features) by the instance's precision, outputs allocated here.  The tests and the tools under tools/ hold each stage against its reference
    # through these; hidden() does not use them (it is one call, ramp_update_forward).  add / add0 = (table, idx): the rows
    # table[idx] of a SoftAgg table, added to the state on the way in.
    def _stage(self, name):
        name = ("ramp_x3_" if self.use_x3 else "ramp_upd_") + name
        fn = getattr(lib(), name)
        return lambda *args: check(fn(*args, stream()), name)

    def corr_mlp(self, corr, net, net_map, inp, inp_idx, inp_mod):
        """LayerNorm((net[net_map] + inp[inp_idx % inp_mod]) + corr-MLP(corr)) for corr [E, 896]; net None: zeros, net_map /
        inp_idx None: row e"""
        w, E = self.weights(), corr.shape[0]
        ln, nm = w["corr_ln"], w["norm"]
        out = torch.empty(E, 384, dtype=torch.float32, device=corr.device)
        self._stage("corr_mlp")(ptr(corr), CORR_ROW, *map(ptr, w["corr1_pack"] + w["tail_pack"]), ptr(ln[0]), ptr(ln[1]),
                                float(ln[2]), ptr(net), ptr(net_map), ptr(inp), ptr(inp_idx), int(inp_mod), ptr(nm[0]),
                                ptr(nm[1]), float(nm[2]), ptr(out), E)
        return out

    def nbr(self, net_in, idx, which, want_t=False):
        """net_in + Lb(relu(La(mask * net_in[idx]))) for the temporal-neighbour MLP `which` = "c1" / "c2" (idx -1: none).
        want_t (fp16 features): also the result's fp16 copy, (out, out_t)"""
        E = net_in.shape[0]
        out = torch.empty_like(net_in)
        out_t = torch.empty(E, 384, dtype=self.dtype, device=net_in.device) if want_t else None
        self._stage("nbr")(ptr(net_in), ptr(idx), *map(ptr, self.weights()[which + "_pack"]), ptr(out),
                           *(() if self.use_x3 else (ptr(out_t),)), E)
        return (out, out_t) if want_t else out

    def fg(self, net32, add_t, add_idx, pack, E, write_back=True):
        """[f(x) | g(x)] [E, 768] for x = net32 (+ add_t[add_idx], written back to net32 unless write_back is off); pack: the
        module's kk_fg_pack / ij_fg_pack"""
        out = torch.empty(E, 768, dtype=self.dtype, device=net32.device)
        self._stage("fg")(ptr(net32), ptr(add_t), ptr(add_idx), ptr(net32) if add_t is not None and write_back else None,
                          *map(ptr, pack), ptr(out), E)
        return out

    def softagg(self, net32, add_t, add_idx, fg_pack, h_pack, groups, max_groups, E):
        """fp16 features: h(segment softmax-sum of f(x), g(x)) for x = net32 (+ add_t[add_idx]) without the [E, 768] rows:
        csrc/update_mlp.hip::upd_softagg_kernel + upd_softagg_finish_kernel"""
        G = max(int(max_groups), 1)
        frag = torch.empty(lib().ramp_upd_softagg_frag_rows(E, G), 3, 384, dtype=torch.float32, device=net32.device)
        self._stage("softagg")(ptr(net32), ptr(add_t), ptr(add_idx), ptr(groups.order), ptr(groups.gid), *map(ptr, fg_pack),
                               ptr(frag), E)
        hy = torch.empty(G, 384, dtype=self.dtype, device=net32.device)
        self._stage("softagg_finish")(ptr(frag), ptr(groups.seg_start), ptr(groups.ngroups), *map(ptr, h_pack), ptr(hy), G)
        return hy

    def h_lin(self, y, pack, groups):
        """SoftAgg's `h` Linear on the group table y, rows below the device-side group count only (fp32 features: the other
        rows are zero); pack: the module's kk_h_pack / ij_h_pack"""
        out = torch.zeros_like(y) if self.use_x3 else torch.empty_like(y)
        self._stage("linear")(ptr(y), *map(ptr, pack), ptr(out), y.shape[0], ptr(groups.ngroups))
        return out

    def gru(self, x32, add=None, add0=None, heads_at=None):
        """gru (LayerNorm, GatedResidual, LayerNorm, GatedResidual) on x = LayerNorm_pre((x32 (+ add0)) + add); without add x32
        is gru[0]'s output already.  add0: fp32 features only (ramp_upd_gru takes one table).  Returns (out32, relu copy in
        self.dtype) -- or, with heads_at = (coords [E,2,P,P], wd, ht), (out32, target, weight) from the launch's epilogue"""
        if add0 is not None and not self.use_x3:
            raise ValueError("FusedUpdate.gru: add0 is the fp32 chains'; the fp16 export takes one table")
        w, E, x3 = self.weights(), x32.shape[0], self.use_x3
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=x32.device)
        ln1, ln2 = w["ln1"], w["ln2"]
        out32 = new(E, 384)
        args = [ptr(x32)] + ([ptr(t) for t in add0 or (None, None)] if x3 else [])
        args += [ptr(add[0]), ptr(add[1]), ptr(ln1[0]), ptr(ln1[1]), float(ln1[2])] if add else [None, None, None, None, 0.0]
        args += [*w["gru_pack"][2:], ptr(ln2[0]), ptr(ln2[1]), float(ln2[2]), ptr(out32)]
        if heads_at is None:
            relu = new(E, 384, dtype=self.dtype)
            self._stage("gru")(*args, ptr(relu), E, *((None,) * 5 + (3, 0.0, 0.0) if x3 else ()))
            return out32, relu
        coords, wd, ht = heads_at
        target, weight = new(1, E, 2), new(1, E, 2)
        heads = [*map(ptr, w["heads_pack"]), ptr(coords), ptr(target), ptr(weight)]
        size = [coords.shape[-1], float(wd), float(ht)]
        self._stage("gru" if x3 else "gru_heads")(*args, *([None, E] + heads if x3 else heads + [E]), *size)
        return out32, target, weight

    def heads_linear(self, relu_t, coords, wd, ht):
        """fp16 features: (target, weight) from the relu copy -- the two heads' Linear layers and ramp_upd_heads's epilogue in one
        launch (csrc/update.hip::upd_heads_linear_f16_kernel)"""
        E = relu_t.shape[0]
        target, weight = (torch.empty(1, E, 2, dtype=torch.float32, device=relu_t.device) for _ in range(2))
        self._stage("heads_linear")(ptr(relu_t), *map(ptr, self.weights()["heads_pack"]), ptr(coords), ptr(target), ptr(weight),
                                    E, coords.shape[-1], float(wd), float(ht))
        return target, weight

    def _hidden_gemm(self, net, inp_table, inp_idx, inp_mod, corr, plan, net_map, net32_buf=None, out32_buf=None):
        """hidden() from library GEMMs (hipBLASLt through torch, bias / bias+ReLU epilogues) and the row kernels of
        csrc/update.hip: every gather, residual add, LayerNorm, gate and dtype cast between two GEMMs is one kernel.  Returns
        (net_out, relu copy); the caller forms the heads.  net32_buf / out32_buf: capacity-sized [>= E, 384] fp32 buffers for
        the state after the first LayerNorm and for the result -- the device-resident fp32 step gathers through index rows
        beyond the live factor count, which must stay inside an allocation."""
        w = self.weights()
        E = corr.shape[0]
        lin, lin_relu, fuse = self.lin, self.lin_relu, self.row_fuse
        # correlation MLP, net + inp + c, LayerNorm (net.py:71-74)
        c = lin(lin_relu(corr, w["corr0_pad"] if corr.shape[1] == CORR_ROW else w["corr0"]), w["corr2"])
        _, c = fuse(E, B=c, ln=w["corr_ln"], relu=True, want_t=True)
        net32, _ = fuse(E, A=net, idxA=net_map, B=inp_table, idxB=inp_idx, modB=inp_mod, C=lin(c, w["corr5"]), ln=w["norm"],
                        want_f32=True, out_f32=net32_buf[:E] if net32_buf is not None else None)
        # temporal neighbours (net.py:77-82); plan.ix_raw / jx_raw keep the -1 markers
        fuse(E, A=net32, B=lin(lin_relu(self.gather_mask(net32, plan.ix_raw, E), w["c1a"]), w["c1b"]), out_f32=net32)
        _, net_t = fuse(E, A=net32, B=lin(lin_relu(self.gather_mask(net32, plan.jx_raw, E), w["c2a"]), w["c2b"]),
                        out_f32=net32, want_t=True)
        # SoftAgg over patches, then over (i, j) pairs (net.py:84-85)
        hy = lin(self.seg(lin(net_t, w["kk_fg"]), plan.g_kk, plan.max_kk), w["kk_h"])
        _, net_t = fuse(E, A=net32, B=hy, idxB32=plan.g_kk.gid, out_f32=net32, want_t=True)
        hy = lin(self.seg(lin(net_t, w["ij_fg"]), plan.g_ij, plan.max_ij), w["ij_h"])
        # gru = LN, GatedResidual, LN, GatedResidual (net.py:49-54)
        x32, x_t = fuse(E, A=net32, B=hy, idxB32=plan.g_ij.gid, ln=w["ln1"], out_f32=net32, want_t=True)
        x32, x_t, _ = self.gated(x32, lin(x_t, w["g1_gate"]), lin(lin_relu(x_t, w["g1_r1"]), w["g1_r2"]), E, ln=w["ln2"],
                                 want_t=True)
        out32, _, relu_t = self.gated(x32, lin(x_t, w["g2_gate"]), lin(lin_relu(x_t, w["g2_r1"]), w["g2_r2"]), E,
                                      want_relu=True, out=out32_buf[:E] if out32_buf is not None else None)
        return out32, relu_t

    # ------------------------------------------------------------------ heads
    def heads(self, relu_t):
        return self.lin(relu_t, self.weights()["heads"])          # [E,4]

    def target_weight(self, hw, coords, wd, ht, want_delta=False):
        E = hw.shape[0]
        P = coords.shape[-1]
        dev = hw.device
        target = torch.empty(1, E, 2, dtype=torch.float32, device=dev)
        weight = torch.empty(1, E, 2, dtype=torch.float32, device=dev)
        delta = torch.empty(1, E, 2, dtype=torch.float32, device=dev) if want_delta else None
        check(lib().ramp_upd_heads(ptr(hw), ptr(coords), ptr(target), ptr(weight), ptr(delta), E, P, float(wd),
                                   float(ht), _code[self.dtype], stream()), "ramp_upd_heads")
        return target, weight, delta
