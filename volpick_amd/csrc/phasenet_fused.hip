// PhaseNet forward, host side: plan_phasenet_fused swaps the 18 layer steps of plan_phasenet for ONE launch
// (pn_window_kernel, phasenet_window.hip: the default) or for the three launches of the reference plans
// (phasenet_tiled.hip: debug dumps, A/B timing).  The packed weights of the layer plan are reused as they are (same
// P / taps / channel padding); what the fused kernels want in another order is packed here.
#include "phasenet_arena.h"

namespace vp {

namespace {

int tensor_id(const Net& net, const std::string& name) {
  for (size_t i = 0; i < net.tensors.size(); ++i)
    if (net.tensors[i].name == name) return (int)i;
  return -1;
}

// [cout = 8][cin][7] (Conv1d) or [cin][cout = 8][7] (ConvTranspose1d) -> [cin][7][8] with the BatchNorm scale folded in:
// channel pairs (2c, 2c + 1) are adjacent, one s_load_dwordx8 fetches a (channel, tap) for all outputs
std::vector<float> pack_valu(const float* W, int cin, bool transposed, const std::vector<float>& scale) {
  std::vector<float> out((size_t)cin * 7 * 8);
  for (int ci = 0; ci < cin; ++ci)
    for (int k = 0; k < 7; ++k)
      for (int co = 0; co < 8; ++co)
        out[((size_t)ci * 7 + k) * 8 + co] = scale[co] * (transposed ? W[((size_t)ci * 8 + co) * 7 + k] : W[((size_t)co * cin + ci) * 7 + k]);
  return out;
}

// up2.same's three-piece operand for one input half (0: skip 1, 1: up2.convT) as 16-channel K-steps (B3Steps<16, 7>: two
// taps per step, tap 7 = zero weights): [step][piece][lane][8], lane = 16 g + row, tap = 2 step + g / 2, channels
// 16 half + 8 (g % 2) ..
std::vector<float> pack_u2same_half(const ConvLayer& L, int half) {
  const int taps = L.g.taps;
  std::vector<uint16_t> o((size_t)4 * 3 * 64 * 8);
  for (int st = 0; st < 4; ++st)
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 8; ++i) {
        const int m = l & 15, g = l >> 4, tap = 2 * st + g / 2, ci = 16 * half + 8 * (g % 2) + i;
        const float w = tap < taps ? L.afrag.h[(((size_t)(ci / 4)) * taps + tap) * 64 + (ci % 4) * 16 + m] : 0.f;
        const size_t base = (((size_t)st * 3) * 64 + l) * 8 + i;
        bf16_split3(w, &o[base], &o[base + 64 * 8], &o[base + 2 * 64 * 8]);
      }
  std::vector<float> f(o.size() / 2);
  memcpy(f.data(), o.data(), o.size() * 2);
  return f;
}

// what the steps share: tensor ids, the debug switches, the VALU weights of the five level-0 layers
struct PnPlan {
  int x, h0, skip0, d0, u2s, u3t;
  bool debug_dumps, debug_clock;
  bool valu;        // the level-0 kernels of the three-launch plan: VALU forms (plan_flags[5] != 1) or all MFMA
  bool persistent;  // the MFMA up3 kernel: two workgroups per window walk the tiles (plan_flags[3] != 1)
  HostBlob *vw[5], *vb[5];  // inc, down0.same, down0.down, up3.convT, up3.same ([cin][7][4] channel pairs, [4] bias pairs); valu only
};

template <class T>
void bind(const Tensor& t, T** p, int* ls, long* ws) {
  *p = t.p;
  *ls = t.ls;
  *ws = (long)t.win_stride();
}
const f32x2* pairs(const HostBlob* b) { return reinterpret_cast<const f32x2*>(b->d); }
const uint4* pieces(const HostBlob* b) { return b ? reinterpret_cast<const uint4*>(b->d) : nullptr; }

double flops(const Net& net, int lo, int hi) {
  double f = 0;
  for (int i = lo; i <= hi; ++i) f += net.convs[i]->flops_per_window;
  return f;
}

Step down0_step(const Net& net, const PnPlan& p) {
  Step st;
  st.name = "fused.down0 (inc+down0.same+down0.down)";
  st.flops_per_window = flops(net, 0, 2);
  st.run = [p](Net& n, int B, hipStream_t s) -> int {
    Down0Args a{};
    bind(n.tensors[p.x], &a.x, &a.ls_x, &a.ws_x);
    bind(n.tensors[p.skip0], &a.skip0, &a.ls_s, &a.ws_s);
    bind(n.tensors[p.d0], &a.d0, &a.ls_d, &a.ws_d);
    if (p.debug_dumps) bind(n.tensors[p.h0], &a.h0_dbg, &a.ls_h, &a.ws_h);
    a.af_inc = n.convs[0]->afrag.d;
    a.bs_inc = n.convs[0]->bias.d;
    a.af_same = n.convs[1]->afrag.d;
    a.bs_same = n.convs[1]->bias.d;
    a.af_down = n.convs[2]->afrag.d;
    a.bs_down = n.convs[2]->bias.d;
    if (!p.valu) {
      pn_launch_down0(a, B, s);
      return 0;
    }
    Down0VArgs v{};
    v.t = a;
    v.w_inc = pairs(p.vw[0]);
    v.b_inc = pairs(p.vb[0]);
    v.w_same = pairs(p.vw[1]);
    v.b_same = pairs(p.vb[1]);
    v.w_down = pairs(p.vw[2]);
    v.b_down = pairs(p.vb[2]);
    v.n_windows = B;
    pn_launch_down0v(v, B, s);
    return 0;
  };
  return st;
}

Step core_step(Net& net, const PnPlan& p) {
  Step st;
  st.name = "fused.core (down1..down4, up0..up2)";
  st.flops_per_window = flops(net, 3, 15);
  static const char* dbg_names[12] = {"down1.same", "down1.down", "down2.same", "down2.down", "down3.same", "down3.down",
                                      "down4.same", "up0.convT",  "up0.same",   "up1.convT",  "up1.same",   "up2.convT"};
  std::vector<int> dbg_ids(12);
  for (int i = 0; i < 12; ++i) dbg_ids[i] = tensor_id(net, dbg_names[i]);
  HostBlob* clk = p.debug_clock ? net.add_blob(std::vector<float>(((size_t)net.max_batch * 32 + 64 * 8) * 2, 0.f)) : nullptr;
  net.debug_clock = clk;
  st.run = [p, dbg_ids, clk](Net& n, int B, hipStream_t s) -> int {
    CoreArgs a{};
    const Tensor &td = n.tensors[p.d0], &tu = n.tensors[p.u2s];
    bind(td, &a.d0, &a.ls_d0, &a.ws_d0);
    bind(tu, &a.u2s, &a.ls_u2s, &a.ws_u2s);
    for (int i = 0; i < 13; ++i) {
      a.af[i] = n.convs[3 + i]->afrag.d;
      a.bs[i] = n.convs[3 + i]->bias.d;
    }
    for (int i = 0; i < 12; ++i)
      if (p.debug_dumps && dbg_ids[i] >= 0) bind(n.tensors[dbg_ids[i]], &a.dbg[i], &a.dbg_ls[i], &a.dbg_ws[i]);
    a.clk = clk ? reinterpret_cast<unsigned long long*>(clk->d) : nullptr;
    a.warm = pf::warm(n.cfg);
    pn_launch_core(a, B, s);
    return 0;
  };
  return st;
}

Step up3_step(Net& net, const PnPlan& p) {
  Step st;
  st.name = "fused.up3 (up3.convT+up3.same+out+softmax)";
  st.flops_per_window = flops(net, 16, 17);
  HostBlob* e0 = &net.convs[17]->e0;
  HostBlob* e1 = &net.convs[17]->e1;
  st.run = [p, e0, e1](Net& n, int B, hipStream_t s) -> int {
    Up3Args a{};
    bind(n.tensors[p.u2s], &a.u2s, &a.ls_u, &a.ws_u);
    bind(n.tensors[p.skip0], &a.skip0, &a.ls_s, &a.ws_s);
    a.y = n.y;
    if (p.debug_dumps) bind(n.tensors[p.u3t], &a.ut_dbg, &a.ls_t, &a.ws_t);
    a.af_t = n.convs[16]->afrag.d;
    a.bs_t = n.convs[16]->bias.d;
    a.af_same = n.convs[17]->afrag.d;
    a.bs_same = n.convs[17]->bias.d;
    a.w_out = e0->d;
    a.b_out = e1->d;
    a.clk = n.debug_clock ? reinterpret_cast<unsigned long long*>(n.debug_clock->d) : nullptr;
    if (!p.valu) {
      pn_launch_up3(a, B, p.persistent && !p.debug_dumps, s);
      return 0;
    }
    Up3VArgs v{};
    v.t = a;
    v.w_t = pairs(p.vw[3]);
    v.b_t = pairs(p.vb[3]);
    v.w_same = pairs(p.vw[4]);
    v.b_same = pairs(p.vb[4]);
    v.n_windows = B;
    pn_launch_up3v(v, B, s);
    return 0;
  };
  return st;
}

// The whole network in one launch.  wd_ids: the debug tensors of a DUMP instance (WD_NAMES), empty without dumps.
Step window_step(Net& net, const PnPlan& p, PnForm form, const std::vector<int>& wd_ids) {
  const bool b3 = form != PnForm::Fp32Core;  // the core layers on bf16 pieces
  const bool d0t = form == PnForm::Default;  // level 0 time-tiled on the matrix cores
  Step st;
  st.name = "fused.window (whole PhaseNet, one workgroup per window)";
  st.flops_per_window = flops(net, 0, 17);
  {  // issued: every layer as whole 16-column tiles of M x (padded channels x taps) on the matrix cores -- as six-MFMA groups
     // over bf16 pieces when b3 (all but the three strided convs), level 0 too when d0t; otherwise inc, down0.same and both
     // halves of up3.same are direct convolutions on the vector ALUs (no padding), like the 1x1 head in every form
    auto padded = [&](int i) {
      const ConvLayer& L = *net.convs[i];
      return 2.0 * L.g.M() * ((L.cols + 15) / 16 * 16) * L.g.cinp() * L.g.taps;
    };
    double f32 = 0, bf16 = 0;
    for (int i = 2; i <= 16; ++i) {
      if (d0t && i == 16) bf16 += (double)U3T_TILES * 8 * 6 * 16384.0;  // up3.convT: 8 (m-tile, n-tile) items per tile x one K-step
      else if (b3 && i >= 7 && i <= 11) bf16 += 6.0 * padded(i);       // down3.same .. up0.same
      else if (b3 && i == 13) bf16 += 6.0 * 2.0 * 32 * 192 * 64 * 7;    // up1.same: 2 m-tiles x 12 n-tiles x 14 K-steps
      else if (b3 && i == 15) bf16 += 6.0 * 2.0 * 16 * 768 * 32 * 8;    // up2.same: 48 n-tiles x 2 halves x 4 K-steps
      else if (b3 && i == 3) bf16 += 48.0 * 2 * 6 * 16384.0;            // down1.same: 48 n-tiles x 2 K-steps
      else if (b3 && i == 5) bf16 += 2.0 * 12 * 4 * 6 * 16384.0;        // down2.same: 2 m-tiles x 12 n-tiles x 4 K-steps
      else if (b3 && i == 12) bf16 += 8.0 * 3 * 4 * 6 * 16384.0;        // up1.convT: 8 m-tiles x 3 n-tiles x 4 K-steps
      else if (b3 && i == 14) bf16 += 4.0 * 12 * 2 * 6 * 16384.0;       // up2.convT: 4 m-tiles x 12 n-tiles x 2 K-steps
      else f32 += padded(i);
    }
    if (d0t) bf16 += (double)D0T_TILES * 16 * (1 + 2) * 6 * 16384.0;  // inc: 96 n-tiles x 1 K-step; down0.same: 96 x 2; six MFMAs each
    if (d0t) bf16 += (double)U3T_TILES * 8 * 4 * 6 * 16384.0;         // up3.same: 8 n-tiles per tile x four K-steps
    // (the 1 x 1 head: 2 x 3 x 8 FLOP per sample on the vector ALUs in every form)
    st.set_issued(f32, bf16, d0t ? 2.0 * 3 * 8 * T0 : flops(net, 0, 1) + flops(net, 17, 17));
  }
  HostBlob* e0 = &net.convs[17]->e0;
  HostBlob* e1 = &net.convs[17]->e1;
  HostBlob* clk = p.debug_clock ? net.debug_clock : nullptr;
  HostBlob* q4[13] = {};
  for (int i = 0; i < 13; ++i)
    if (q4_layer_index(i)) q4[i] = net.add_blob(regroup_afrag4(*net.convs[3 + i]));
  // three-piece operands (WindowArgs names the layers)
  HostBlob *p3[6] = {}, *p3d12[2] = {}, *p3inc = nullptr, *p3d0s = nullptr, *p3u3t = nullptr, *p3u3s = nullptr, *p3uT[2] = {}, *p3u2[2] = {};
  if (b3) {
    for (int i = 0; i < 5; ++i) p3[i] = net.add_blob(b3_operand(*net.convs[3 + 4 + i], i == 3));
    p3[5] = net.add_blob(b3_operand(*net.convs[3 + 10], false));
    p3d12[0] = net.add_blob(b3_operand(*net.convs[3 + 0], false));
    p3d12[1] = net.add_blob(b3_operand(*net.convs[3 + 2], false));
  }
  if (d0t) {
    p3inc = net.add_blob(b3_operand(*net.convs[0], true));
    p3d0s = net.add_blob(b3_operand(*net.convs[1], true));
    p3u3t = net.add_blob(b3_operand(*net.convs[16], true));
    p3u3s = net.add_blob(b3_operand(*net.convs[17], true));
  }
  if (b3) {
    p3uT[0] = net.add_blob(b3_operand(*net.convs[3 + 9], true));
    p3uT[1] = net.add_blob(b3_operand(*net.convs[3 + 11], true));
    for (int half = 0; half < 2; ++half) p3u2[half] = net.add_blob(pack_u2same_half(*net.convs[3 + 12], half));
  }
  st.run = [=](Net& n, int B, hipStream_t s) -> int {
    WindowArgs a{};
    for (int i = 0; i < 13; ++i) a.af4[i] = q4[i] ? q4[i]->d : nullptr;
    for (int i = 0; i < 2; ++i) {
      a.af3_d12[i] = pieces(p3d12[i]);
      a.af3_uT[i] = pieces(p3uT[i]);
      a.af3_u2[i] = pieces(p3u2[i]);
    }
    a.af3_inc = pieces(p3inc);
    a.af3_d0s = pieces(p3d0s);
    a.bs_inc8 = n.convs[0]->bias.d;
    a.bs_d0s = n.convs[1]->bias.d;
    a.af3_u3t = pieces(p3u3t);
    a.af3_u3s = pieces(p3u3s);
    a.bs_u3t = n.convs[16]->bias.d;
    a.bs_u3s = n.convs[17]->bias.d;
    for (int i = 0; i < 6; ++i) {
      a.af3[i] = pieces(p3[i]);
      a.af3_lines[i] = p3[i] ? (int)(p3[i]->h.size() * 4 / 128) : 0;
    }
    for (int i = 0; i < 13; ++i) {
      a.c.af[i] = n.convs[3 + i]->afrag.d;
      a.c.bs[i] = n.convs[3 + i]->bias.d;
    }
    a.c.clk = clk ? reinterpret_cast<unsigned long long*>(clk->d) : nullptr;
    a.c.warm = pf::warm(n.cfg) && n.warm_launches > 0;
    if (n.warm_launches > 0) --n.warm_launches;
    bind(n.tensors[p.x], &a.x, &a.ls_x, &a.ws_x);
    bind(n.tensors[p.skip0], &a.skip0, &a.ls_s, &a.ws_s);
    a.y = n.y;
    a.w_inc = pairs(p.vw[0]);
    a.b_inc = pairs(p.vb[0]);
    a.w_same = pairs(p.vw[1]);
    a.b_same = pairs(p.vb[1]);
    a.w_up = pairs(p.vw[4]);
    a.b_up = pairs(p.vb[4]);
    a.af_down = n.convs[2]->afrag.d;
    a.bs_down = n.convs[2]->bias.d;
    a.af_t = n.convs[16]->afrag.d;
    a.bs_t = n.convs[16]->bias.d;
    a.w_out = e0->d;
    a.b_out = e1->d;
    if (n.pre) {
      a.pre = *n.pre;
      a.has_pre = 1;
    }
    for (size_t i = 0; i < wd_ids.size(); ++i) bind(n.tensors[wd_ids[i]], &a.dbg[i], &a.dbg_ls[i], &a.dbg_ws[i]);
    pn_launch_window(form, !wd_ids.empty(), a, B, s);
    return 0;
  };
  return st;
}

}  // namespace

int plan_phasenet_fused(Net& net, const ParamView& pv, int debug_flags) {
  PnPlan p{};
  p.debug_dumps = (debug_flags & pf::DBG_LDS_DUMPS) != 0;
  p.debug_clock = (debug_flags & pf::DBG_CLOCK) != 0;
  // bit 2: the one-launch kernel's DUMP instance writes every layer's output (and the head's logits) to the debug tensors
  const bool win_dumps = (debug_flags & pf::DBG_LAYER_DUMPS) != 0;
  const int f5 = pf::get(net.cfg, pf::PN_FORM);
  if (win_dumps && (p.debug_dumps || f5 != pf::PN_DEFAULT || pf::get(net.cfg, pf::PRE) != 0)) {
    set_error("PhaseNet plan_flags[1] & 4 dumps the default one-launch form only (plan_flags[1] & 1, plan_flags[5], plan_flags[6] unset)");
    return VP_ERR_UNSUPPORTED;
  }
  // Removed in round 6: the hand-pipelined K loop and the intermediate forms of pn_window_kernel between its references
  if (pf::get(net.cfg, pf::MID) == pf::MID_PN_REMOVED || pf::pn_form_removed(f5)) {
    set_error("PhaseNet plan_flags[2] = %d / plan_flags[5] = %d: this A/B form was removed in round 6 (kept: plan_flags[5] = 0, 1, 2, 3, 8)",
              pf::get(net.cfg, pf::MID), f5);
    return VP_ERR_UNSUPPORTED;
  }
  if (pf::get(net.cfg, pf::TILES) == pf::TILES_PN_REMOVED) {
    set_error("PhaseNet plan_flags[3] = 2 (persistent level-0 down kernel): removed in round 6");
    return VP_ERR_UNSUPPORTED;
  }
  // plan_flags[5] = 1: the three-launch plan with the MFMA forms of the two level-0 kernels (bit-identical to the layer plan),
  // 2: with their VALU forms; otherwise the whole network in one launch, in one of three forms.  The debug dumps of
  // plan_flags[1] & 1 exist in the three-launch plans only.
  p.valu = f5 != pf::PN_TILED_MFMA;
  p.persistent = pf::get(net.cfg, pf::TILES) != pf::TILES_ALT;  // plan_flags[3] = 1: one workgroup per tile for up3 too (A/B timing)
  const bool whole = p.valu && f5 != pf::PN_TILED_VALU && !p.debug_dumps;
  const PnForm form = f5 == pf::PN_FP32_CORE ? PnForm::Fp32Core : f5 == pf::PN_LEVEL0_VALU ? PnForm::Level0Valu : PnForm::Default;
  if (p.valu) {
    const float eps = net.cfg.bn_eps;
    struct {
      const char *conv, *bn;
      int cin;
      bool transposed, bias;
    } spec[5] = {{"inc", "in_bn", 3, false, true},
                 {"down_branch.0.0", "down_branch.0.1", 8, false, false},
                 {"down_branch.0.2", "down_branch.0.3", 8, false, false},
                 {"up_branch.3.0", "up_branch.3.1", 16, true, false},
                 {"up_branch.3.2", "up_branch.3.3", 16, false, false}};
    for (int i = 0; i < 5; ++i) {
      std::vector<float> scale, shift;
      bn_fold(pv, spec[i].bn, 8, eps, spec[i].bias ? pv.get(std::string(spec[i].conv) + ".bias") : nullptr, &scale, &shift);
      p.vw[i] = net.add_blob(pack_valu(pv.get(std::string(spec[i].conv) + ".weight"), spec[i].cin, spec[i].transposed, scale));
      p.vb[i] = net.add_blob(shift);
    }
  }
  if (net.convs.size() != 18) {
    set_error("fused PhaseNet plan expects the 18-layer plan");
    return VP_ERR_INVALID;
  }
  p.x = net.input;
  p.h0 = tensor_id(net, "inc");
  p.skip0 = tensor_id(net, "down0.same");
  p.d0 = tensor_id(net, "down0.down");
  p.u2s = tensor_id(net, "up2.same");
  p.u3t = tensor_id(net, "up3.convT");
  // furthest reads of the tiled loaders
  net.need(p.x, (N_TILES - 1) * TT - 8 + 4 * ((TT + 28) / 4));
  net.need(p.skip0, HALO + (N_TILES - 1) * TT - 16 + 12 + 4 * 130);
  net.need(p.u2s, HALO + (N_TILES - 1) * TT / 4 - 4 + 144);
  if (p.valu) {
    net.need(p.x, HALO + VD_TS * (VD_TILES - 1) - 12 + VS);      // x image float4 loads
    net.need(p.skip0, VU_TS * (VU_TILES - 1) + VS);              // skip image float4 loads
    net.need(p.skip0, HALO + VD_TS * VD_TILES);                  // skip stores of the last down tile
    net.need(p.u2s, HALO + (VU_TS / 4) * (VU_TILES - 1) - 2 + 258);  // up2.same image loads
    net.need(p.x, HALO - 4 + W0_S);      // whole-window float4 loads of pn_window_kernel
    net.need(p.skip0, HALO - 4 + W0_S);
  }
  std::vector<int> wd_ids;
  if (win_dumps) {  // up3.same and the head's logits exist in registers only: tensors of their own for the dumps
    net.add_tensor("up3.same", 8, T0);
    net.add_tensor("logits", 3, T0);
    for (int i = 0; i < WD_COUNT; ++i) {
      wd_ids.push_back(tensor_id(net, WD_NAMES[i]));
      if (wd_ids[i] < 0) {
        set_error("PhaseNet dumps: no tensor %s", WD_NAMES[i]);
        return VP_ERR_INVALID;
      }
    }
  }
  std::vector<Step> steps;
  steps.push_back(down0_step(net, p));
  steps.push_back(core_step(net, p));
  steps.push_back(up3_step(net, p));
  if (whole) {
    steps.clear();
    steps.push_back(window_step(net, p, form, wd_ids));
    net.fused_pre = pf::get(net.cfg, pf::PRE) != pf::PRE_PN_GATHER;  // plan_flags[6] = 1: gather_normalize_kernel fills the input tensor as in the other plans
    net.fused_pre_poisons = true;                // ... and then writes the NaN predictions of a non-finite window itself
    pn_register_window(net, win_dumps);
  }
  net.steps = std::move(steps);
  pn_register_tiled(net);
  return VP_OK;
}

}  // namespace vp
