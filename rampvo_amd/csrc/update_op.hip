// The update operator (ramp/net.py:69-90) as ONE launch sequence: the correlation MLP, the two neighbour chains, the two
// SoftAggs and the gru with the heads.  ramp_track_step (csrc/track.hip) and ramp_update_forward (the host-driven tracker,
// rampvo_amd/update_fused.py) both run ramp_i_update_operator; the kernels are csrc/update_mlp.hip's (fp16 features) and
// csrc/update_x3.hip's (fp32 features).
#include "ramp_device.h"
#include "ramp_internal.h"

#define UPD_DO(call)                \
  do {                              \
    const int rc_ = (call);         \
    if (rc_ != RAMP_OK) return rc_; \
  } while (0)

int ramp_i_update_check(const UpdOp &op) {
  const ramp_update_args &a = op.a;
  const ramp_track_weights *w = a.w;
  if (!w || a.E < 0 || a.kk_cap <= 0 || a.ij_cap <= 0) return RAMP_EINVAL;
  const void *const need[] = {
      w->corr_w1, w->corr_w2, w->corr_w3, w->corr_b1, w->corr_b2, w->corr_b3, w->corr_ln_w, w->corr_ln_b, w->norm_w, w->norm_b,
      w->c1_wa, w->c1_wb, w->c2_wa, w->c2_wb, w->c1_ba, w->c1_bb, w->c2_ba, w->c2_bb, w->kk_wf, w->kk_wg, w->kk_wh, w->ij_wf,
      w->ij_wg, w->ij_wh, w->kk_bf, w->kk_bg, w->kk_bh, w->ij_bf, w->ij_bg, w->ij_bh, w->ln1_w, w->ln1_b, w->ln2_w, w->ln2_b,
      a.corr, a.inp, a.state[0], a.state[1], a.net_out, a.kk_order, a.kk_gid, a.kk_seg, a.kk_ngroups, a.ij_order, a.ij_gid,
      a.ij_seg, a.ij_ngroups, a.ix, a.jx, a.hkk, a.hij};
  for (const void *p : need)
    if (!p) return RAMP_EINVAL;
  for (int i = 0; i < 6; i++)
    if (!w->gru_w[i] || !w->gru_b[i]) return RAMP_EINVAL;
  if (a.fp32 ? (!a.fg || !a.ykk || !a.yij) : !a.sagg_frag) return RAMP_EINVAL;
  // the heads' operands come as a group; without them the relu copy is the result the caller's heads read
  const bool heads = a.coords != nullptr;
  if (heads ? (!a.target || !a.weight || !w->heads_w || !w->heads_b || a.P < 1) : (a.target || a.weight || !a.relu_out))
    return RAMP_EINVAL;
  if (a.state[0] == a.state[1] || a.net_prev == a.state[0]) return RAMP_EINVAL;
  return RAMP_OK;
}

int ramp_i_update_operator(const UpdOp &op, hipStream_t st) {
  const ramp_update_args &a = op.a;
  const ramp_track_weights &w = *a.w;
  const int E = a.E;
  float *s0 = a.state[0], *s1 = a.state[1];
  if (E == 0) return RAMP_OK;
  auto h16 = [](const void *p) { return (const _Float16 *)p; };
  // The stages' operand records (update_params.h), filled by name.  A twin pair (fp16 / fp32 features) names its fields alike, so
  // one generic filler serves both; what only one of them has is set where it is launched.
  auto corr_mlp = [&](auto p) {
    p.corr = (decltype(p.corr))a.corr; p.corr_k = 896;
    p.w1 = h16(w.corr_w1); p.b1 = w.corr_b1; p.w2 = h16(w.corr_w2); p.b2 = w.corr_b2; p.w3 = h16(w.corr_w3); p.b3 = w.corr_b3;
    p.ln_w = w.corr_ln_w; p.ln_b = w.corr_ln_b; p.ln_eps = w.corr_ln_eps;
    p.net = a.net_prev; p.net_map = a.net_map;
    p.inp = (decltype(p.inp))a.inp; p.inp_idx = a.inp_idx; p.inp_mod = a.inp_mod;
    p.norm_w = w.norm_w; p.norm_b = w.norm_b; p.norm_eps = w.norm_eps;
    p.net_out = s0; p.E = E; p.dyn = op.dyn;
    return p;
  };
  // c1: s0 -> s1 through the ii neighbours, c2: s1 -> s0 through the jj neighbours
  auto nbr = [&](auto p, bool c2) {
    p.net_in = c2 ? s1 : s0; p.idx = c2 ? a.jx : a.ix; p.net_out = c2 ? s0 : s1;
    p.wa = h16(c2 ? w.c2_wa : w.c1_wa); p.ba = c2 ? w.c2_ba : w.c1_ba;
    p.wb = h16(c2 ? w.c2_wb : w.c1_wb); p.bb = c2 ? w.c2_bb : w.c1_bb;
    p.E = E; p.dyn = op.dyn;
    return p;
  };
  // the f and g layers of a SoftAgg on s0: over the patch groups, or (ij) over the pair groups, which read net + hkk[patch group]
  auto agg_fg = [&](auto p, bool ij) {
    p.x32 = s0;
    if (ij) { p.add_t = (decltype(p.add_t))a.hkk; p.add_idx = a.kk_gid; }
    p.wf = h16(ij ? w.ij_wf : w.kk_wf); p.bf = ij ? w.ij_bf : w.kk_bf;
    p.wg = h16(ij ? w.ij_wg : w.kk_wg); p.bg = ij ? w.ij_bg : w.kk_bg;
    p.E = E; p.dyn = op.dyn;
    return p;
  };
  // gru on (s0 + hkk[patch group]) + hij[pair group], with the heads in its epilogue when the caller gave coords
  auto gru = [&](auto p) {
    p.E = E; p.dyn = op.dyn;
    p.x32 = s0;
    p.add0_t = (decltype(p.add0_t))a.hkk; p.add0_idx = a.kk_gid;
    p.add_t = (decltype(p.add_t))a.hij; p.add_idx = a.ij_gid;
    p.pre_w = w.ln1_w; p.pre_b = w.ln1_b; p.pre_eps = w.ln1_eps;
    upd_gru_layers(p, w.gru_w, w.gru_b);
    p.ln_w = w.ln2_w; p.ln_b = w.ln2_b; p.eps = w.ln2_eps;
    p.out32 = a.net_out;
    p.heads_w = a.coords ? (decltype(p.heads_w))w.heads_w : nullptr; p.heads_b = w.heads_b;
    p.coords = a.coords; p.target = a.target; p.weight = a.weight;
    upd_patch_side(p, a.P);
    p.wd = a.wd; p.ht = a.ht;
    return p;
  };
  if (a.fp32) {
    // csrc/update_x3.hip's chains (Linear layers on the f16 matrix cores from split fp32 operands), fp32 tables,
    // [f | g] rows + segment softmax + h for the two SoftAggs
    float *hkk = (float *)a.hkk, *hij = (float *)a.hij;
    UPD_DO(ramp_i_x3_corr_mlp(corr_mlp(X3CorrMlpParams{}), st));
    UPD_DO(ramp_i_x3_nbr(nbr(X3NbrParams{}, false), st));
    UPD_DO(ramp_i_x3_nbr(nbr(X3NbrParams{}, true), st));
    X3FgParams fg = agg_fg(X3FgParams{}, false);
    fg.fg = a.fg;
    UPD_DO(ramp_i_x3_fg(fg, st));
    UPD_DO(ramp_x3_segment_softmax(a.fg, a.kk_order, a.kk_seg, a.kk_ngroups, a.ykk, a.kk_cap, st));
    UPD_DO(ramp_x3_linear(a.ykk, w.kk_wh, w.kk_bh, hkk, a.kk_cap, a.kk_ngroups, st));
    fg = agg_fg(X3FgParams{}, true);
    fg.fg = a.fg;
    UPD_DO(ramp_i_x3_fg(fg, st));
    UPD_DO(ramp_x3_segment_softmax(a.fg, a.ij_order, a.ij_seg, a.ij_ngroups, a.yij, a.ij_cap, st));
    UPD_DO(ramp_x3_linear(a.yij, w.ij_wh, w.ij_bh, hij, a.ij_cap, a.ij_ngroups, st));
    X3GruParams g = gru(X3GruParams{});
    g.relu32 = (float *)a.relu_out;
    return ramp_i_x3_gru(g, st);
  }
  // the fp16 fused chains of csrc/update_mlp.hip
  UPD_DO(ramp_i_upd_corr_mlp(corr_mlp(CorrTailParams{}), st));
  UPD_DO(ramp_i_upd_nbr(nbr(NbrParams{}, false), st));
  UPD_DO(ramp_i_upd_nbr(nbr(NbrParams{}, true), st));
  // the next frame's front end may start here, before the first SoftAgg (against before the gru chain, rounds 2-3: +1.2 %
  // SingleScale, +2.1 % MultiScale -- the front end costs the operator ~25 us and gives bundle adjustment 12 back).  The
  // "go" is the word the first SoftAgg launch's first workgroup stores (gate_flag), or else the caller's event.
  if (!op.gate_flag && op.gate_event && hipEventRecord((hipEvent_t)op.gate_event, st) != hipSuccess) return RAMP_ELAUNCH;
  // SoftAgg x 2 (ramp/net.py:84-85): gather-by-group tiles, g and f on the same tile, online softmax in registers, h on
  // the merged fragments -- 2 launches each, no [E, 768] rows.  The pair SoftAgg reads net + hkk[patch group] and does not
  // write the sum back: the gru launch forms (net + hkk[.]) + hij[.] itself (tests/test_update_operator_gpu.py pins that
  // this equals the written-back sum bit for bit)
  SoftAggParams kk = agg_fg(SoftAggParams{}, false);
  kk.order = a.kk_order; kk.gid = a.kk_gid; kk.frag = a.sagg_frag; kk.gate_flag = op.gate_flag; kk.gate_seq = op.gate_seq;
  UPD_DO(ramp_i_upd_softagg(kk, st));
  UPD_DO(ramp_upd_softagg_finish(a.sagg_frag, a.kk_seg, a.kk_ngroups, w.kk_wh, w.kk_bh, a.hkk, a.kk_cap, st));
  SoftAggParams ij = agg_fg(SoftAggParams{}, true);
  ij.order = a.ij_order; ij.gid = a.ij_gid; ij.frag = a.sagg_frag;
  UPD_DO(ramp_i_upd_softagg(ij, st));
  UPD_DO(ramp_upd_softagg_finish(a.sagg_frag, a.ij_seg, a.ij_ngroups, w.ij_wh, w.ij_bh, a.hij, a.ij_cap, st));
  // (the heads and target / weight are formed in the gru launch's epilogue: no relu(net) round trip, one launch less)
  GruParams g = gru(GruParams{});
  g.relu_t = (_Float16 *)a.relu_out;
  return ramp_i_upd_gru(g, a.E_hint, st);
}

extern "C" int ramp_update_forward(const ramp_update_args *args, void *stream) {
  if (!args || args->E < 0) return RAMP_EINVAL;
  if (args->E == 0) return RAMP_OK;
  const UpdOp op = {*args, nullptr, nullptr, nullptr, 0};
  UPD_DO(ramp_i_update_check(op));
  return ramp_i_update_operator(op, (hipStream_t)stream);
}
