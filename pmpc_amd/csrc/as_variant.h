// as_variant.h — which instantiation of k_bwd_as / k_fwd_as (kernels_as.hip) a launch takes, and which instantiations exist.
// The ONE place where the variants of the active-set sweeps are chosen and listed.  Plain C++ (no HIP): the launchers of
// kernels_as.hip call the selectors and guard every instantiation with the predicates; pmpc_as_sweep_variant (include/pmpc_abi.h)
// shows both to a test that needs no device (tests/test_as_variant.py).
#pragma once

// PMPC_AS_DEEP2_MAXM, PMPC_AS_DEEP_MAXM, PMPC_AS_FWD_PF2_MAXM: the launcher reads them once per process
struct AsSweepKnobs { int deep2_maxm, deep_maxm, fwd_pf2_maxm; };

// template arguments of k_bwd_as: MODE (0 lean, 1 deep, 2 deep2), SKIP, DEFECT, EX (0 none, 1 cone, 2 state box), MT = float
struct BwdAsVariant { int mode; bool skip, defect; int ex; bool f32; };
// template arguments of k_fwd_as: DEFECT, PF2, CONE, MT = float, SENS
struct FwdAsVariant { bool defect, pf2, cone, f32, sens; };

// What the launch carries: M particles on this rank, and which of LQArgs' defect, as_settled_in, mat32, cone_H, xb_D are set.
constexpr BwdAsVariant select_bwd_as(int M, bool defect, bool settled_in, bool mat32, bool cone_H, bool xb_D, const AsSweepKnobs &k) {
  BwdAsVariant v = {};
  v.f32 = mat32;
  v.ex = cone_H ? 1 : (xb_D && !mat32 ? 2 : 0);  // fp32 > cone > state box: an fp32 sweep carries cones, but DROPS the state-box terms
  v.defect = defect;
  v.skip = settled_in && !defect;                 // (the first round has nothing to skip)
  const bool plain = !v.f32 && v.ex == 0;
  // waves per SIMD this launch brings (1024 SIMDs): <= 2 deep2, <= 3 deep, else lean (see k_bwd_as)
  v.mode = M <= k.deep2_maxm ? 2 : (M <= k.deep_maxm ? 1 : 0);
  if (v.mode == 0 && defect) v.mode = 1;          // never lean with DEFECT: the deep variant needs 127 registers, 4 waves per SIMD without help
  if (v.mode == 0 && !plain) v.mode = 1;          // never lean with cones / state boxes / fp32 (one more register per prefetch set)
  // SKIP, few particles left: the latency regime at every M.  Only the plain family listens to deep2_maxm = 0 ("never deep2")
  if (v.skip) v.mode = (plain && k.deep2_maxm <= 0) ? 1 : 2;
  return v;
}

// Index of a variant in the launch counts (pmpc_as_sweep_launches, include/pmpc_abi.h states the layout): one code per record
constexpr int AS_BWD_CODES = 72, AS_FWD_CODES = 32;
constexpr int bwd_as_code(const BwdAsVariant &v) { return v.mode + 3 * (v.skip + 2 * (v.defect + 2 * (v.ex + 3 * v.f32))); }
constexpr int fwd_as_code(const FwdAsVariant &v) { return v.defect + 2 * v.pf2 + 4 * v.cone + 8 * v.f32 + 16 * v.sens; }

// cone + SENS + DEFECT is the one forward sweep on the one-stage ring, whatever the knob says (registers)
constexpr bool fwd_as_one_stage_only(bool defect, bool cone, bool sens) { return defect && cone && sens; }

// What the launch carries: M, the consensus horizon Nc, and which of LQArgs' defect, mat32, as_uraw, as_T are set.
constexpr FwdAsVariant select_fwd_as(int M, int Nc, bool defect, bool mat32, bool as_uraw, bool as_T, const AsSweepKnobs &k) {
  FwdAsVariant v = {};
  v.defect = defect;
  v.f32 = mat32;
  v.cone = as_uraw;                               // (the record of the unclamped step is what the cone rounds add to this sweep)
  v.sens = as_T && Nc == 1;                       // SENS only with one consensus stage
  const bool plain = !v.f32 && !v.cone && !v.sens;
  // two-stage prefetch everywhere (+0.8 % at 4096 particles); fwd_pf2_maxm puts larger launches of the PLAIN family back on the
  // one-stage ring, every other family ignores it
  v.pf2 = plain ? M <= k.fwd_pf2_maxm : !fwd_as_one_stage_only(v.defect, v.cone, v.sens);
  return v;
}

// (xdim, udim) pairs of PMPC_FAST_DIMS with fp32-storage / cone / state-box instantiations of the sweeps
constexpr bool as_f32_dims(int XD, int UD) { return (XD == 12 && UD == 4) || (XD == 6 && UD == 3) || (XD == 4 && UD == 2); }
constexpr bool as_cone_dims(int XD, int UD) { return UD >= 2; }
constexpr bool as_xbox_dims(int XD, int UD) { return true; }

// Which k_bwd_as<XD, UD, ..> exist.  Per family (plain, cone, state box; fp32 plain, fp32 cone): MODE 1 and 2 with and without
// DEFECT, SKIP with MODE 2.  The plain family alone also has SKIP with MODE 1 and the lean MODE 0 — the latter with DEFECT too,
// which select_bwd_as never asks for.
constexpr bool bwd_as_compiled(const BwdAsVariant &v, int XD, int UD) {
  if (v.f32 && !(as_f32_dims(XD, UD) && v.ex != 2)) return false;
  if (v.ex == 1 && !as_cone_dims(XD, UD)) return false;
  if (v.ex == 2 && !as_xbox_dims(XD, UD)) return false;
  const bool plain = !v.f32 && v.ex == 0;
  if (v.skip) return !v.defect && (v.mode == 2 || (plain && v.mode == 1));
  return v.mode != 0 || plain;
}

// Which k_fwd_as<XD, UD, ..> exist: the plain family on both rings, every other on the ring its selection rule names.
constexpr bool fwd_as_compiled(const FwdAsVariant &v, int XD, int UD) {
  if (v.f32 && !as_f32_dims(XD, UD)) return false;
  if (v.cone && !as_cone_dims(XD, UD)) return false;
  const bool plain = !v.f32 && !v.cone && !v.sens;
  return plain || v.pf2 == !fwd_as_one_stage_only(v.defect, v.cone, v.sens);
}
