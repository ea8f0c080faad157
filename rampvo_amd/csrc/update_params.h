// The operand records of the update operator's stages: each is the ONE argument of its kernel (csrc/update_mlp.hip: fp16
// features, csrc/update_x3.hip: fp32 features) and of its launcher (ramp_i_upd_* / ramp_i_x3_*, csrc/ramp_internal.h).  Callers
// fill them by field name -- csrc/update_op.hip from ramp_update_args / ramp_track_weights, the exported ramp_upd_* / ramp_x3_*
// from their positional arguments -- and the launcher validates what it finds.  The fp16 and fp32 twins stay apart: their
// field orders differ, and the order is the kernels' argument layout.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- fp16 features (csrc/update_mlp.hip)
struct GruParams {
  const float *x32;            // [E][384] fp32: the LayerNorm'ed residual stream entering gru[1]
  const _Float16 *wp[6];       // packed weights: g1_gate, g1_r1, g1_r2, g2_gate, g2_r1, g2_r2
  const float *bias[6];        // biases (fp16-rounded values as fp32)
  const float *ln_w, *ln_b;    // gru[2] LayerNorm
  float eps;
  float *out32;                // [E][384] fp32 result of gru[3]
  _Float16 *relu_t;            // [E][384] relu(result) in fp16 (input of the heads)
  // optional prologue: x = LayerNorm_pre(x32 + add_t[add_idx]) -- the last SoftAgg's expand-and-add and gru[0]
  const _Float16 *add_t;       // [groups][384] fp16 or NULL
  const int32_t *add_idx;      // [E]
  const _Float16 *add0_t;      // optional: a FIRST expand-and-add (x32 + add0_t[add0_idx]) + add_t[add_idx] -- the second-last
  const int32_t *add0_idx;     // SoftAgg's, when the launch that consumed it did not write the sum back
  const float *pre_w, *pre_b;  // gru[0] LayerNorm
  float pre_eps;
  int E;
  const int32_t *dyn;          // optional device-side sizes (RAMP_DYN_*): E is then the launch bound
  // optional epilogue: the two heads and target / weight (ramp/net.py:87-90, ramp/Ramp_vo.py:291-297) from the
  // result tile while it is in registers -- relu_t is then not written (may be NULL)
  const _Float16 *heads_w;     // [4][384] fp16: d.weight rows 0..1, w.weight rows 0..1
  const float *heads_b;        // [4]
  const float *coords;         // [E][2][PP]
  float *target, *weight;      // [E][2]
  int PP, ctr;                 // (upd_patch_side)
  float wd, ht;
};

struct NbrParams {
  const float *net_in;         // [E][384] fp32
  const int64_t *idx;          // [E] neighbour row or -1
  const _Float16 *wa, *wb;     // packed weights of the two Linear layers
  const float *ba, *bb;        // biases (fp16-rounded values as fp32)
  float *net_out;              // [E][384] fp32, must not alias net_in
  _Float16 *out_t;             // optional [E][384] fp16 copy of net_out
  int E;
  const int32_t *dyn;          // optional device-side sizes (RAMP_DYN_*): E is then the launch bound
};

struct CorrTailParams {
  // FULL variant: the first Linear (+ReLU) of the MLP on the correlation rows as well
  const _Float16 *corr;        // [E][corr_k] fp16 (corr_k a multiple of 32, e.g. 896 = 882 + zero padding)
  const _Float16 *w1;          // packed [corr_k/32][24][64][8]
  const float *b1;
  int corr_k;
  const _Float16 *c1;          // [E][384] fp16 (tail-only variant: relu(Linear1(corr)) from a library GEMM)
  const _Float16 *w2, *w3;     // packed weights of corr[2], corr[5]
  const float *b2, *b3;        // biases (fp16-rounded values as fp32)
  const float *ln_w, *ln_b;    // corr[3] LayerNorm
  float ln_eps;
  const float *net;            // [*][384] fp32 previous hidden state or NULL (zeros)
  const int64_t *net_map;      // [E] row of `net` per edge (-1: zero row) or NULL (identity)
  const _Float16 *inp;         // context table [*][384] fp16
  const int64_t *inp_idx;      // [E] row of `inp` (taken modulo inp_mod when inp_mod > 0) or NULL (identity)
  long inp_mod;
  const float *norm_w, *norm_b;
  float norm_eps;
  float *net_out;              // [E][384] fp32, must not alias net
  int E;
  const int32_t *dyn;          // optional device-side sizes (RAMP_DYN_*): E is then the launch bound
};

struct FgParams {
  const float *x32;            // [E][384] fp32
  const _Float16 *add_t;       // optional [groups][384] fp16
  const int32_t *add_idx;      // [E]
  float *x32_out;              // optional [E][384] fp32 (may be x32): x after the add
  const _Float16 *wf, *wg;     // packed weights of f and g
  const float *bf, *bg;        // biases (fp16-rounded values as fp32)
  _Float16 *fg;                // [E][768] fp16
  int E;
  const int32_t *dyn;          // optional device-side sizes (RAMP_DYN_*): E is then the launch bound
};

struct SoftAggParams {
  const float *x32;            // [E][384] fp32
  const _Float16 *add_t;       // optional [groups'][384] fp16: x = x32 + add_t[add_idx] (the previous SoftAgg's expand-and-add)
  const int32_t *add_idx;      // [E]
  const int32_t *order;        // [E] sorted position -> factor
  const int32_t *gid;          // [E] factor -> group
  const _Float16 *wf, *wg;     // packed weights of f and g
  const float *bf, *bg;        // biases (fp16-rounded values as fp32)
  float *frag;                 // [slots][3][384] fp32: (m, z, a) per run
  int E;
  const int32_t *dyn;          // optional device-side sizes (RAMP_DYN_*): E is then the launch bound
  uint32_t *gate_flag;         // optional: workgroup 0 stores gate_seq here when it starts (ramp_track.gate_flag)
  uint32_t gate_seq;
};

// ---- fp32 features (csrc/update_x3.hip): weights are x3 packs, everything else float
struct X3NbrParams {
  const float *net_in;         // [E][384]
  const int64_t *idx;          // [E] neighbour row or -1
  const _Float16 *wa, *wb;     // packed (x3)
  const float *ba, *bb;        // fp32 biases
  float *net_out;              // [E][384], must not alias net_in
  int E;
  const int32_t *dyn;
};

struct X3CorrMlpParams {
  const float *corr;           // [E][corr_k] fp32 (corr_k a multiple of 32: 896 = 882 + zero tail)
  int corr_k;
  const _Float16 *w1, *w2, *w3;
  const float *b1, *b2, *b3;
  const float *ln_w, *ln_b;    // corr[3]
  float ln_eps;
  const float *net;            // [*][384] previous hidden state or NULL (zeros)
  const int64_t *net_map;      // [E] row of `net` per factor (-1: zero row) or NULL (identity)
  const float *inp;            // context table [*][384] fp32
  const int64_t *inp_idx;      // [E] row of `inp` (modulo inp_mod when > 0) or NULL (identity)
  long inp_mod;
  const float *norm_w, *norm_b;
  float norm_eps;
  float *net_out;              // [E][384], must not alias net
  int E;
  const int32_t *dyn;
};

struct X3FgParams {
  const float *x32;            // [E][384]
  const float *add_t;          // optional [groups][384] fp32: x = x32 + add_t[add_idx]
  const int32_t *add_idx;
  float *x32_out;              // optional: x written back (may be x32)
  const _Float16 *wf, *wg;
  const float *bf, *bg;
  float *fg;                   // [E][768] fp32
  int E;
  const int32_t *dyn;
};

struct X3LinParams {
  const float *x;              // [rows][384]
  const _Float16 *w;
  const float *b;
  float *y;                    // [rows][384]
  int E;                       // rows (launch bound)
  const int32_t *rows_dev;     // optional device-side row count
  const int32_t *dyn;          // unused (X3_COMMON)
};

struct X3GruParams {
  const float *x32;            // [E][384]: the residual stream entering gru[0]
  const float *add0_t;         // optional first expand-and-add table (fp32) -- (x32 + add0_t[add0_idx]) + add_t[add_idx]
  const int32_t *add0_idx;
  const float *add_t;          // optional: with it x = LayerNorm_pre(x32 (+ add0) + add_t[add_idx]) (gru[0]); without: x = x32
  const int32_t *add_idx;
  const float *pre_w, *pre_b;
  float pre_eps;
  const _Float16 *wp[6];       // g1_gate, g1_r1, g1_r2, g2_gate, g2_r1, g2_r2 (x3 packs)
  const float *bias[6];
  const float *ln_w, *ln_b;    // gru[2]
  float eps;
  float *out32;                // [E][384]
  float *relu32;               // optional [E][384]: relu(result)
  const float *heads_w;        // optional [4][384] fp32 (d rows 0..1, w rows 0..1) -> target / weight
  const float *heads_b;        // [4]
  const float *coords;         // [E][2][PP]
  float *target, *weight;      // [E][2]
  int PP, ctr;                 // (upd_patch_side)
  float wd, ht;
  int E;
  const int32_t *dyn;
};

// ---- what the two gru records share (host code)
// the heads' view of a P x P patch: its size and its centre element.  P < 1 leaves PP = 0, which the launchers refuse
template <class GruT>
static inline void upd_patch_side(GruT &p, int P) {
  p.PP = P < 1 ? 0 : P * P;
  p.ctr = (P / 2) * P + P / 2;
}
// the six Linear layers of the two GatedResiduals from a caller's pointer arrays, once p.E is set: a missing array leaves null
// entries, which the launchers refuse, and without rows the arrays are not read (E <= 0 is answered before any pointer)
template <class GruT>
static inline void upd_gru_layers(GruT &p, const void *const *w, const float *const *b) {
  for (int i = 0; i < 6 && p.E > 0; i++) {
    p.wp[i] = w ? (const _Float16 *)w[i] : nullptr;
    p.bias[i] = b ? b[i] : nullptr;
  }
}
