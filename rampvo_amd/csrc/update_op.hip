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
  const int32_t *dyn = op.dyn;
  float *s0 = a.state[0], *s1 = a.state[1];
  const void *heads_w = a.coords ? w.heads_w : nullptr;
  if (E == 0) return RAMP_OK;
  if (a.fp32) {
    // csrc/update_x3.hip's chains (Linear layers on the f16 matrix cores from split fp32 operands), fp32 tables,
    // [f | g] rows + segment softmax + h for the two SoftAggs
    float *fg = a.fg, *hkk = (float *)a.hkk, *hij = (float *)a.hij;
    UPD_DO(ramp_i_x3_corr_mlp((const float *)a.corr, 896, w.corr_w1, w.corr_b1, w.corr_w2, w.corr_b2, w.corr_w3, w.corr_b3,
                              w.corr_ln_w, w.corr_ln_b, w.corr_ln_eps, a.net_prev, a.net_map, (const float *)a.inp, a.inp_idx,
                              a.inp_mod, w.norm_w, w.norm_b, w.norm_eps, s0, E, dyn, st));
    UPD_DO(ramp_i_x3_nbr(s0, a.ix, w.c1_wa, w.c1_ba, w.c1_wb, w.c1_bb, s1, E, dyn, st));
    UPD_DO(ramp_i_x3_nbr(s1, a.jx, w.c2_wa, w.c2_ba, w.c2_wb, w.c2_bb, s0, E, dyn, st));
    UPD_DO(ramp_i_x3_fg(s0, nullptr, nullptr, nullptr, w.kk_wf, w.kk_bf, w.kk_wg, w.kk_bg, fg, E, dyn, st));
    UPD_DO(ramp_x3_segment_softmax(fg, a.kk_order, a.kk_seg, a.kk_ngroups, a.ykk, a.kk_cap, st));
    UPD_DO(ramp_x3_linear(a.ykk, w.kk_wh, w.kk_bh, hkk, a.kk_cap, a.kk_ngroups, st));
    UPD_DO(ramp_i_x3_fg(s0, hkk, a.kk_gid, nullptr, w.ij_wf, w.ij_bf, w.ij_wg, w.ij_bg, fg, E, dyn, st));
    UPD_DO(ramp_x3_segment_softmax(fg, a.ij_order, a.ij_seg, a.ij_ngroups, a.yij, a.ij_cap, st));
    UPD_DO(ramp_x3_linear(a.yij, w.ij_wh, w.ij_bh, hij, a.ij_cap, a.ij_ngroups, st));
    return ramp_i_x3_gru(s0, hkk, a.kk_gid, hij, a.ij_gid, w.ln1_w, w.ln1_b, w.ln1_eps, w.gru_w, w.gru_b, w.ln2_w, w.ln2_b,
                         w.ln2_eps, a.net_out, (float *)a.relu_out, E, dyn, (const float *)heads_w, w.heads_b, a.coords,
                         a.target, a.weight, a.P, a.wd, a.ht, st);
  }
  // the fp16 fused chains of csrc/update_mlp.hip
  UPD_DO(ramp_i_upd_corr_mlp(a.corr, 896, w.corr_w1, w.corr_b1, w.corr_w2, w.corr_b2, w.corr_w3, w.corr_b3, w.corr_ln_w,
                             w.corr_ln_b, w.corr_ln_eps, a.net_prev, a.net_map, a.inp, a.inp_idx, a.inp_mod, w.norm_w,
                             w.norm_b, w.norm_eps, s0, E, dyn, st));
  UPD_DO(ramp_i_upd_nbr(s0, a.ix, w.c1_wa, w.c1_ba, w.c1_wb, w.c1_bb, s1, nullptr, E, dyn, st));
  UPD_DO(ramp_i_upd_nbr(s1, a.jx, w.c2_wa, w.c2_ba, w.c2_wb, w.c2_bb, s0, nullptr, E, dyn, st));
  // the next frame's front end may start here, before the first SoftAgg (against before the gru chain, rounds 2-3: +1.2 %
  // SingleScale, +2.1 % MultiScale -- the front end costs the operator ~25 us and gives bundle adjustment 12 back).  The
  // "go" is the word the first SoftAgg launch's first workgroup stores (gate_flag), or else the caller's event.
  if (!op.gate_flag && op.gate_event && hipEventRecord((hipEvent_t)op.gate_event, st) != hipSuccess) return RAMP_ELAUNCH;
  // SoftAgg x 2 (ramp/net.py:84-85): gather-by-group tiles, g and f on the same tile, online softmax in registers, h on
  // the merged fragments -- 2 launches each, no [E, 768] rows.  The pair SoftAgg reads net + hkk[patch group] and does not
  // write the sum back: the gru launch forms (net + hkk[.]) + hij[.] itself (tests/test_update_operator_gpu.py pins that
  // this equals the written-back sum bit for bit)
  UPD_DO(ramp_i_upd_softagg(s0, nullptr, nullptr, a.kk_order, a.kk_gid, w.kk_wf, w.kk_bf, w.kk_wg, w.kk_bg, a.sagg_frag, E,
                            dyn, st, op.gate_flag, op.gate_seq));
  UPD_DO(ramp_upd_softagg_finish(a.sagg_frag, a.kk_seg, a.kk_ngroups, w.kk_wh, w.kk_bh, a.hkk, a.kk_cap, st));
  UPD_DO(ramp_i_upd_softagg(s0, a.hkk, a.kk_gid, a.ij_order, a.ij_gid, w.ij_wf, w.ij_bf, w.ij_wg, w.ij_bg, a.sagg_frag, E, dyn,
                            st));
  UPD_DO(ramp_upd_softagg_finish(a.sagg_frag, a.ij_seg, a.ij_ngroups, w.ij_wh, w.ij_bh, a.hij, a.ij_cap, st));
  // (the heads and target / weight are formed in the gru launch's epilogue: no relu(net) round trip, one launch less)
  return ramp_i_upd_gru(s0, a.hkk, a.kk_gid, a.hij, a.ij_gid, w.ln1_w, w.ln1_b, w.ln1_eps, w.gru_w, w.gru_b, w.ln2_w, w.ln2_b,
                        w.ln2_eps, a.net_out, a.relu_out, E, dyn, heads_w, w.heads_b, a.coords, a.target, a.weight, a.P, a.wd,
                        a.ht, a.E_hint, st);
}

extern "C" int ramp_update_forward(const ramp_update_args *args, void *stream) {
  if (!args || args->E < 0) return RAMP_EINVAL;
  if (args->E == 0) return RAMP_OK;
  const UpdOp op = {*args, nullptr, nullptr, nullptr, 0};
  UPD_DO(ramp_i_update_check(op));
  return ramp_i_update_operator(op, (hipStream_t)stream);
}
