// jac_compact.h — compact Jacobian records of the built-in models (dynamics.hip writes them, the active-set sweeps of
// kernels_as.hip read them, k_expand_jac turns them back into the dense ABI stacks).
//
// Most entries of a built-in model's fx / fu are structural: 0, 1, dt, or a constant of the particle (dt / Jx ...).  A model
// declares the class of every entry as a picture (Spec::ROWS, one string per row: the X columns of fx, then the U columns of
// fu); everything else here is derived from that picture at compile time.
//   'x'          live: depends on the state or the control, stored per (particle, stage)
//   '.'          structural zero
//   other chars  a constant of the particle, named in Spec::CONSTS ('1', 'd' = dt, 'a' = dt / Jx ...); its value is taken from
//                the first entry of that class the model evaluates, so it is the very double the dense stack holds
//
// The sweeps read the Jacobians as TRIPLES of KS = X / 4 consecutive entries, in two orientations (fast_common.h, Lane):
//   factor sweep   rows KS g .. KS g + KS - 1 of a column   (column triple)
//   forward sweep  columns KS g .. KS g + KS - 1 of a row   (row triple), and single entries fu[row][g]
// Record of one (particle, stage) unit, REC doubles: every column triple with a live entry (fx columns in order, then fu's),
// then every row triple of fx with a live entry — whole triples, their constant entries included, so a lane reads KS
// consecutive doubles.  A live single entry of fu is read inside its column triple.
// Constant pool of one particle, POOL doubles: KS zeros, then each constant followed by KS - 1 zeros.  A triple without a live
// entry has at most one non-zero entry (checked below), so it IS a window of the pool: the lane points there with stage stride 0.
// Buffer: [M N records | M pools], in the caller's fx scratch array (X X doubles per unit: always enough).
#pragma once

namespace jacc {

constexpr int NONE = -(1 << 30);  // lane map: this lane reads no Jacobian entry

struct UnicycleSpec {
  static constexpr int X = 4, U = 2, MODEL = 0;  // MODEL: the id of the ABI (include/pmpc_abi.h)
  static constexpr const char *CONSTS = "1ab";  // 1, T v_scale, -T w_scale
  static constexpr const char *ROWS[4] = {
      "1.xx" "xx",
      ".1xx" "xx",
      "..1." "a.",
      "...1" ".b",
  };
};
struct BicycleSpec {
  static constexpr int X = 4, U = 2, MODEL = 2;
  static constexpr const char *CONSTS = "1d";  // 1, dt
  static constexpr const char *ROWS[4] = {
      "1.xx" "..",
      ".1xx" "..",
      "..1x" ".x",
      "...1" "d.",
  };
};
struct QuadrotorSpec {
  static constexpr int X = 12, U = 4, MODEL = 1;
  static constexpr const char *CONSTS = "1dabc";  // 1, dt, dt / Jx, dt / Jy, dt / Jz
  static constexpr const char *ROWS[12] = {
      "1..d........" "....",
      ".1..d......." "....",
      "..1..d......" "....",
      "...1..xxx..." "x...",
      "....1.xxx..." "x...",
      ".....1xx...." "x...",
      "......xx.dxx" "....",
      "......x1..xx" "....",
      "......xx1.xx" "....",
      ".........1xx" ".a..",
      ".........x1x" "..b.",
      ".........xx1" "...c",
  };
};

template <class S>
struct Compact {
  static constexpr int X = S::X, U = S::U, KS = X / 4, XX = X * X, XU = X * U;
  static_assert(X == 4 * KS, "compact records: xdim must be a multiple of 4 (no padded lanes)");
  static constexpr int cstrlen(const char *s) { int n = 0; while (s[n]) n++; return n; }
  static constexpr int NCONST = cstrlen(S::CONSTS);
  static constexpr int POOL = KS + KS * NCONST;
  // class of entry (r, c) of [fx | fu]: -1 live, 0 zero, k >= 1 constant CONSTS[k - 1]
  static constexpr int cls(int r, int c) {
    const char ch = S::ROWS[r][c];
    if (ch == 'x') return -1;
    if (ch == '.') return 0;
    for (int k = 0; k < NCONST; k++) if (S::CONSTS[k] == ch) return k + 1;
    return -1000;  // (unknown character: caught by the static_assert below)
  }
  static constexpr int pool_of(int k) { return k == 0 ? 0 : KS + KS * (k - 1); }  // pool index of constant class k (0: a zero)
  // window of the pool that equals a triple without live entries (-1000: two non-zero entries, not representable)
  static constexpr int pool_window(const int (&k)[4]) {
    int at = -1;
    for (int r = 0; r < KS; r++) if (k[r] != 0) { if (at >= 0) return -1000; at = r; }
    return at < 0 ? 0 : pool_of(k[at]) - at;
  }
  struct Tables {
    int rec = 0;                // doubles per record
    bool ok = true;
    int col[(X + U) * 4] = {};  // column triple (column c of [fx | fu], row block g): record offset, or -1 - pool window
    int row[X * 4] = {};        // row triple (row r of fx, column block g): likewise
    int rec_src[(X + U) * X * 2] = {};  // record slot -> index into the dense unit [fx (column-major) | fu (column-major)]
    int pool_src[POOL] = {};    // pool slot -> dense index of the entry its value comes from, -1: zero
    int bwd[64] = {}, fwdA[64] = {}, fwdB[64] = {};  // per-lane maps of the sweeps (lane layout of fast_common.h)
    int expand[2][XX + XU] = {};  // dense index -> source, read through the column (0) / row (1) oriented part of the record
  };
  static constexpr Tables build() {
    Tables t;
    for (int k = 0; k < POOL; k++) t.pool_src[k] = -1;
    for (int c = 0; c < X + U; c++)
      for (int r = 0; r < X; r++) {
        const int k = cls(r, c);
        if (k == -1000) t.ok = false;
        if (k >= 1 && t.pool_src[pool_of(k)] < 0) t.pool_src[pool_of(k)] = r + X * c;
      }
    for (int c = 0; c < X + U; c++)
      for (int g = 0; g < 4; g++) {
        int k[4] = {0, 0, 0, 0};
        bool live = false;
        for (int r = 0; r < KS; r++) { k[r] = cls(KS * g + r, c); live |= k[r] == -1; }
        if (live) {
          t.col[c * 4 + g] = t.rec;
          for (int r = 0; r < KS; r++) t.rec_src[t.rec++] = (KS * g + r) + X * c;
        } else {
          const int w = pool_window(k);
          if (w == -1000) t.ok = false;
          t.col[c * 4 + g] = -1 - w;
        }
      }
    for (int r = 0; r < X; r++)
      for (int g = 0; g < 4; g++) {
        int k[4] = {0, 0, 0, 0};
        bool live = false;
        for (int q = 0; q < KS; q++) { k[q] = cls(r, KS * g + q); live |= k[q] == -1; }
        if (live) {
          t.row[r * 4 + g] = t.rec;
          for (int q = 0; q < KS; q++) t.rec_src[t.rec++] = r + X * (KS * g + q);
        } else {
          const int w = pool_window(k);
          if (w == -1000) t.ok = false;
          t.row[r * 4 + g] = -1 - w;
        }
      }
    // single entry (r, c) of [fx | fu] through the column-oriented part
    auto single_col = [&](int r, int c) {
      const int m = t.col[c * 4 + r / KS];
      return m >= 0 ? m + r % KS : (cls(r, c) >= 0 ? -1 - pool_of(cls(r, c)) : NONE);
    };
    auto single_row = [&](int r, int c) {
      if (c >= X) return single_col(r, c);  // (fu has no row-oriented copy)
      const int m = t.row[r * 4 + c / KS];
      return m >= 0 ? m + c % KS : (cls(r, c) >= 0 ? -1 - pool_of(cls(r, c)) : NONE);
    };
    for (int c = 0; c < X + U; c++)
      for (int r = 0; r < X; r++) {
        t.expand[0][r + X * c] = single_col(r, c);
        t.expand[1][r + X * c] = single_row(r, c);
        if (t.expand[0][r + X * c] == NONE || t.expand[1][r + X * c] == NONE) t.ok = false;
      }
    for (int lane = 0; lane < 64; lane++) {  // (Lane<X, U> of fast_common.h)
      const int c = lane & 15, g = lane >> 4, oc = (c & 3) * KS + (c >> 2), cb = c - X;
      const bool cxv = c < X && oc < X, cu = cb >= 0 && cb < U;
      t.bwd[lane] = cxv ? t.col[oc * 4 + g] : (cu ? t.col[(X + cb) * 4 + g] : NONE);
      t.fwdA[lane] = cxv ? t.row[oc * 4 + g] : NONE;
      t.fwdB[lane] = (cxv && g < U) ? single_col(oc, X + g) : NONE;
    }
    return t;
  }
  static constexpr Tables tab = build();
  static_assert(tab.ok, "compact records: unknown class character, or a constant triple with two non-zero entries");
  static constexpr int REC = tab.rec;
  static_assert(REC + POOL <= XX, "compact records must fit the fx scratch array for every horizon N >= 1");
};

// The models whose records a sweep instantiation (XD, UD) can read: the dimensions do not name the model, LQArgs::jac_compact does
// (model id + 1).  select() gives a lane its entries of the three maps and the record / pool sizes of the candidate with that id —
// one uniform branch per further candidate, in the prologue of the sweep; a pair with one candidate takes it without a test.
template <class... S> struct SpecList { static constexpr int COUNT = sizeof...(S); };
template <int XD, int UD> struct SpecFor { typedef SpecList<> list; };
template <> struct SpecFor<4, 2> { typedef SpecList<UnicycleSpec, BicycleSpec> list; };
template <> struct SpecFor<12, 4> { typedef SpecList<QuadrotorSpec> list; };

struct LaneSel { int bwd, fwdA, fwdB, rec, pool; };
template <class S0, class... S>
__device__ __forceinline__ LaneSel select(SpecList<S0, S...>, int tag, int lane) {
  if constexpr (sizeof...(S) > 0) {
    if (tag != S0::MODEL + 1) return select(SpecList<S...>{}, tag, lane);
  }
  typedef Compact<S0> C;
  return {C::tab.bwd[lane], C::tab.fwdA[lane], C::tab.fwdB[lane], C::REC, C::POOL};
}

}  // namespace jacc
