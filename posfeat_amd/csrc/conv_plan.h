// conv_plan.h -- launch planning of the conv / batched-GEMM family (conv.hip)
// as a pure function: (ConvShape, ConvMode) -> Plan.  Plain C++: no HIP, no
// globals, no environment, so the planner runs and is checked on the host
// alone (tests/host/conv_plan_check.cpp).  conv.hip captures the ambient state
// into a ConvMode once per call (conv_mode()) and launches Plan::variant.
//
// One Plan decides kernel, tile and split for a conv so the launch, the
// split-K workspace and the stats reduction agree on the tiling.
#pragma once
#include <climits>
#include <cmath>

constexpr int CONV_BK = 32;  // K chunk of every conv kernel

enum ConvKern { KERN_STAGED = 0, KERN_GLDS = 1, KERN_HALO = 2 };
// Tile ids: stored in records/tile_db.txt, taken by POSFEAT_CONV_TILE and the
// planes ABI's tile argument -- never renumber.
enum ConvTile {
  TILE_128x128 = 0, TILE_128x64 = 1, TILE_64x64 = 2, TILE_256x128 = 3,
  TILE_H8x128 = 10, TILE_H8x64 = 11, TILE_H16x128 = 12,
  TILE_BF6_128x128 = 20, TILE_BF6_128x256 = 21, TILE_BF6_64x128 = 22, TILE_BF6_128x64 = 23,
  TILE_BF6B_128x128 = 24, TILE_BF6B_128x64 = 25, TILE_BF6R_128x128 = 26, TILE_BF6R_128x64 = 27,
  TILE_BF6B_256x128 = 28, TILE_BF6X_128x128 = 29, TILE_BF6X_128x64 = 30, TILE_BF6X_256x128 = 31,
  TILE_BF6X_128x192 = 32, TILE_BF6X_128x256 = 33, TILE_BF6X_192x128 = 34, TILE_BF6X_256x64 = 35
};
enum ConvArith { CONV_ARITH_FP32 = 0, CONV_ARITH_BF6 = 1 };

// What the planner reads of a conv.  GEMM view: M = n * OH * OW output
// pixels (hw = OH * OW per image), N = Cout, K = KH * KW * Cin padded to Kpad.
// Every field is positive (pad >= 0) and hw and Kpad fit an int, so KH * KW and
// the patch counts below do; sums and products with M or Cout are formed in
// 64 bits (cdiv) and the grid is range-checked (plan_launch).
struct ConvShape {
  long long M;
  int hw, OH, OW, Cin, xcs, Cout, KH, KW, stride, pad, Kpad;
  bool has_wb;     // weights also as three bf16 planes
  bool has_xb;     // A pre-split by its producer (pf_gemm_batched_pre)
  bool has_x2;     // two-source 1x1 GEMM (pf_conv_dual)
  bool has_amean;  // A normalised on load (pf_conv_run_tile_np)
};

// Everything ambient: the precision (posfeat_set_conv_precision), the calling
// thread's scopes and the A/B switches (POSFEAT_<name>; the defaults are the
// shipped choice, the only one the shipped library runs).
struct ConvMode {
  int precision = 1;       // 0 fp32 MFMA, 1 bf16x6, 2 bf16x6 + producer-split operands
  bool halo_fp32 = false;  // PfHaloFp32Scope(true)
  bool dense32 = false;    // PfDense32Scope, PfHaloFp32Scope(false)
  bool stem32 = false;     // PfHaloFp32Scope(false)
  bool bf6_halo = true;    // BF6_HALO=0: the 3x3 stride-1 halo kernel in fp32 MFMA
  int bf6d = 2;            // BF6D: A prefetch depth 2..4 of conv_bf6d_kernel, 0: conv_bf6b_kernel
  bool bf6x = true;        // BF6X=0: dense / gather convs on the 32x32x16 tiles
  bool bf6_stem = true;    // BF6_STEM=0: the Cin = 4 staged convs in fp32 MFMA
  int maxsplit = 4;        // CONV_MAXSPLIT
  int kmax = KERN_HALO;    // CONV_KERNEL=staged|glds caps the kernel family
  int tile = -1;           // POSFEAT_CONV_TILE: a tile forced where legal
  bool bm192 = false;      // BF6X_BM192=1: dense / two-source 128x128 plans run 192x128
  bool rb4n64 = false;     // BF6X_RB4N64=1: dense / stem 128x64 plans run 256x64
  // pf_gemm_batched
  bool gemm_b256 = false;        // GEMM_B256=1: the 8-wave 256x128 pre-split tiles
  bool rb4 = false;              // BF6X_RB4=1: 256-row 16x16x32 tiles
  bool n256 = false;             // BF6X_N256=1: one 256-wide column tile for N % 256 == 0
  bool train_wino_bf6x = false;  // TRAIN_WINO_BF6X=1: halo scope lifted for the batched GEMMs
  int wsb = 3;  // WSB: weight-stationary batched GEMMs, 0 off, 1 K = 192, 2 K <= 192, 3 all

  // bf16x6 products (fp32-exact, see split3) for every conv the row-tile DMA
  // kernels serve.  The candidate set of a conv is all-bf16x6 or all-fp32 and
  // one arithmetic within it, so the autotuner's choice never changes results.
  bool bf6_on() const { return precision >= 1; }
  // the halo kernel in bf16x6 too; PfHaloFp32Scope keeps the train-mode
  // backbone on the fp32 halo tiles its fp64-pinned fixtures were validated on
  bool halo_bf6_on() const { return bf6_on() && bf6_halo && !halo_fp32; }
  // dense / gather convs on the 16x16x32 conv_bf6x_kernel: its sums are not
  // bit-identical to the 32x32x16 tiles', which the training scopes keep
  // 
  bool bf6x_on() const { return bf6_on() && bf6x && !halo_fp32 && !dense32; }
  // the Cin = 4 register-staged convs in bf16x6
  bool stem_bf6_on() const { return bf6_on() && bf6_stem && !halo_fp32 && !stem32; }
};

// ---------------------------------------------------------------------------
// The tile table: one row per tile id.
enum TileFamily {
  FAM_ROWS,       // contiguous rows, fp32 MFMA: staged (conv_mfma_kernel) or DMA (conv_glds_kernel)
  FAM_ROWS_GLDS,  // ... DMA only
  FAM_HALO,       // ph x 16 pixel patches of 3x3 stride-1 convs (conv_halo_kernel)
  FAM_BF6,        // rows, bf16x6, operands split in the kernel (conv_glds_kernel)
  FAM_BF6B,       // + pre-split weights (conv_bf6s / conv_bf6d / conv_bf6b_kernel)
  FAM_BF6R,       // + A straight to registers (conv_bf6d_kernel; masked taps too)
  FAM_BF6X        // pre-split weights, 16x16x32 MFMAs (conv_bf6x_kernel)
};
// the convs a bf6x tile serves
enum { XK_DENSE = 1, XK_GT = 2, XK_G4 = 4, XK_DUAL = 8 };

struct TileRow {
  int id;
  const char* name;
  int family;
  int bm, bn;       // output rows x columns per workgroup (halo: bm = ph * 16)
  int ph;           // patch height (halo), else 0
  int threads;      // per workgroup
  int cout_div;     // Cout % cout_div == 0 required (0: any)
  int xkinds;       // FAM_BF6X: XK_* it serves
  const char* not_candidate;  // null: an autotune candidate; else why not
};

// Candidates are offered to the autotuner in table order.
constexpr TileRow kTileTable[] = {
    {TILE_H8x128, "H8x128", FAM_HALO, 128, 128, 8, 256, 128, 0, nullptr},
    {TILE_H8x64, "H8x64", FAM_HALO, 128, 64, 8, 256, 0, 0, nullptr},
    {TILE_H16x128, "H16x128", FAM_HALO, 256, 128, 16, 512, 128, 0,
     "A/B only: POSFEAT_CONV_TILE=12 makes it the default halo tile"},
    {TILE_128x128, "128x128", FAM_ROWS, 128, 128, 0, 256, 0, 0, nullptr},
    {TILE_128x64, "128x64", FAM_ROWS, 128, 64, 0, 256, 0, 0, nullptr},
    {TILE_64x64, "64x64", FAM_ROWS, 64, 64, 0, 256, 0, 0, nullptr},
    {TILE_256x128, "256x128", FAM_ROWS_GLDS, 256, 128, 0, 512, 128, 0, nullptr},
    {TILE_BF6_128x128, "BF6_128x128", FAM_BF6, 128, 128, 0, 256, 0, 0, nullptr},
    {TILE_BF6_128x256, "BF6_128x256", FAM_BF6, 128, 256, 0, 256, 256, 0, nullptr},
    {TILE_BF6_64x128, "BF6_64x128", FAM_BF6, 64, 128, 0, 256, 0, 0, nullptr},
    {TILE_BF6_128x64, "BF6_128x64", FAM_BF6, 128, 64, 0, 256, 0, 0, nullptr},
    {TILE_BF6B_128x128, "BF6B_128x128", FAM_BF6B, 128, 128, 0, 256, 0, 0, nullptr},
    {TILE_BF6B_128x64, "BF6B_128x64", FAM_BF6B, 128, 64, 0, 256, 0, 0, nullptr},
    {TILE_BF6R_128x128, "BF6R_128x128", FAM_BF6R, 128, 128, 0, 256, 0, 0, nullptr},
    {TILE_BF6R_128x64, "BF6R_128x64", FAM_BF6R, 128, 64, 0, 256, 0, 0, nullptr},
    // 8 waves stacked along M (one 135-KB block per CU); Cout > 64 only
    {TILE_BF6B_256x128, "BF6B_256x128", FAM_BF6B, 256, 128, 0, 512, 0, 0, nullptr},
    {TILE_BF6X_128x128, "BF6X_128x128", FAM_BF6X, 128, 128, 0, 256, 0, XK_DENSE | XK_GT, nullptr},
    {TILE_BF6X_128x64, "BF6X_128x64", FAM_BF6X, 128, 64, 0, 256, 0, XK_DENSE | XK_GT | XK_G4,
     nullptr},
    // head.conv1's Winograd GEMMs, the tap GEMM: A read once per 192 columns
    {TILE_BF6X_128x192, "BF6X_128x192", FAM_BF6X, 128, 192, 0, 256, 192, XK_DENSE, nullptr},
    {TILE_BF6X_256x128, "BF6X_256x128", FAM_BF6X, 256, 128, 0, 256, 0, XK_DENSE | XK_GT,
     "never faster; timing noise let it take the tap GEMM at +5 % (r7i)"},
    {TILE_BF6X_128x256, "BF6X_128x256", FAM_BF6X, 128, 256, 0, 256, 256, XK_DENSE,
     "A/B only: the batched GEMMs' choice under POSFEAT_BF6X_N256=1"},
    // six waves stacked along M: the B tile's L2 -> CU bytes per output 2/3
    {TILE_BF6X_192x128, "BF6X_192x128", FAM_BF6X, 192, 128, 0, 384, 0, XK_DENSE | XK_DUAL,
     "A/B only: replaces 128x128 plans under POSFEAT_BF6X_BM192=1"},
    // RB = 4: half the B bytes per output
    {TILE_BF6X_256x64, "BF6X_256x64", FAM_BF6X, 256, 64, 0, 256, 0, XK_DENSE | XK_G4,
     "A/B only: replaces 128x64 plans under POSFEAT_BF6X_RB4N64=1"},
};

inline const TileRow* tile_row(int tile) {
  for (const TileRow& r : kTileTable)
    if (r.id == tile) return &r;
  return nullptr;
}

// ---------------------------------------------------------------------------
// The kernel instantiations conv_run launches: X(variant, kernel).  A variant's
// name is its kernel expression.  (The staged forms of the DMA-only 256x128
// row tile are never planned; they stay listed with their siblings.)
#define CONV_ROW_VARIANTS(X, T, BM, BN, WM, WN)                       \
  X(V_ROWS_##T##_GLDS, (conv_glds_kernel<BM, BN, WM, WN>))             \
  X(V_ROWS_##T##_MFMA32, (conv_mfma_kernel<BM, BN, WM, WN, true>))     \
  X(V_ROWS_##T##_STEM_BF6, (conv_mfma_kernel<BM, BN, WM, WN, false, true>)) \
  X(V_ROWS_##T##_STEM_FP32, (conv_mfma_kernel<BM, BN, WM, WN, false>))
#define CONV_VARIANTS(X)                                          \
  CONV_ROW_VARIANTS(X, 128x128, 128, 128, 2, 2)                   \
  CONV_ROW_VARIANTS(X, 128x64, 128, 64, 2, 2)                     \
  CONV_ROW_VARIANTS(X, 64x64, 64, 64, 2, 2)                       \
  CONV_ROW_VARIANTS(X, 256x128, 256, 128, 4, 2)                   \
  X(V_H8x128_FP32, (conv_halo_kernel<8, 128, 2, 2, 3, 3>))        \
  X(V_H8x128_BF6, (conv_halo_kernel<8, 128, 2, 2, 3, 3, true>))   \
  X(V_H8x64_FP32, (conv_halo_kernel<8, 64, 2, 2, 3, 3>))          \
  X(V_H8x64_BF6, (conv_halo_kernel<8, 64, 2, 2, 3, 3, true>))     \
  X(V_H16x128_FP32, (conv_halo_kernel<16, 128, 4, 2, 3, 3>))      \
  X(V_BF6_128x128, (conv_glds_kernel<128, 128, 2, 2, 2, true>))   \
  X(V_BF6_128x256, (conv_glds_kernel<128, 256, 2, 2, 2, true>))   \
  X(V_BF6_64x128, (conv_glds_kernel<64, 128, 2, 2, 2, true>))     \
  X(V_BF6_128x64, (conv_glds_kernel<128, 64, 2, 2, 2, true>))     \
  X(V_BF6S_128x128, (conv_bf6s_kernel<128, 128, 2>))              \
  X(V_BF6S_128x64, (conv_bf6s_kernel<128, 64, 2>))                \
  X(V_BF6D2_128x128, (conv_bf6d_kernel<128, 128, 2>))             \
  X(V_BF6D3_128x128, (conv_bf6d_kernel<128, 128, 3>))             \
  X(V_BF6D4_128x128, (conv_bf6d_kernel<128, 128, 4>))             \
  X(V_BF6D2_128x64, (conv_bf6d_kernel<128, 64, 2>))               \
  X(V_BF6D3_128x64, (conv_bf6d_kernel<128, 64, 3>))               \
  X(V_BF6D4_128x64, (conv_bf6d_kernel<128, 64, 4>))               \
  X(V_BF6D2_256x128, (conv_bf6d_kernel<256, 128, 2, 8>))          \
  X(V_BF6D3_256x128, (conv_bf6d_kernel<256, 128, 3, 8>))          \
  X(V_BF6B_128x128, (conv_bf6b_kernel<128, 128>))                 \
  X(V_BF6B_128x64, (conv_bf6b_kernel<128, 64>))                   \
  X(V_BF6B_256x128, (conv_bf6b_kernel<256, 128, 8>))              \
  X(V_X128_DENSE, (conv_bf6x_kernel<128>))                        \
  X(V_X128_GT, (conv_bf6x_kernel<128, 2, 2>))                     \
  X(V_X128_DUAL, (conv_bf6x_kernel<128, 2, 3>))                   \
  X(V_X128_NORM, (conv_bf6x_kernel<128, 2, 4>))                   \
  X(V_X64_DENSE, (conv_bf6x_kernel<64>))                          \
  X(V_X64_G4, (conv_bf6x_kernel<64, 2, 1>))                       \
  X(V_X64_GT, (conv_bf6x_kernel<64, 2, 2>))                       \
  X(V_X192_DENSE, (conv_bf6x_kernel<192>))                        \
  X(V_X256_DENSE, (conv_bf6x_kernel<256>))                        \
  X(V_X64_RB4_DENSE, (conv_bf6x_kernel<64, 4>))                   \
  X(V_X64_RB4_G4, (conv_bf6x_kernel<64, 4, 1>))                   \
  X(V_X128_NW6_DENSE, (conv_bf6x_kernel<128, 2, 0, 6>))           \
  X(V_X128_NW6_DUAL, (conv_bf6x_kernel<128, 2, 3, 6>))            \
  X(V_X128_RB4_DENSE, (conv_bf6x_kernel<128, 4>))                 \
  X(V_X128_RB4_GT, (conv_bf6x_kernel<128, 4, 2>))

enum ConvVariant {
  V_NONE = -1,
#define CONV_X(V, K) V,
  CONV_VARIANTS(CONV_X)
#undef CONV_X
  V_COUNT
};
inline const char* variant_name(int v) {
  static const char* const names[] = {
#define CONV_X(V, K) #K,
      CONV_VARIANTS(CONV_X)
#undef CONV_X
  };
  return v >= 0 && v < V_COUNT ? names[v] : "none";
}

struct Plan {
  // the planned tile: what the split-K and stats workspaces are sized by
  int kern, tile, bm, bn, ppi;  // kern < 0: illegal; ppi: patches per image (halo), 0 = rows
  long long tiles_m;
  int ksplit;
  // the launch (plan_launch): variant == V_NONE if the grid does not fit an int
  int run_tile;  // = tile, or its BM192 / RB4N64 substitute
  int variant, threads, tiles_n, nwg, arith;
};

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// 1x1, no padding, any stride (a strided 1x1 conv is a GEMM over the
// subsampled pixel rows: conv_bf6x_kernel maps each row to its input pixel)
inline bool dense_gemm(const ConvShape& s) {
  return s.KH == 1 && s.KW == 1 && s.pad == 0 && s.has_wb && !s.has_xb;
}
// Cin % 32 == 0 convs with taps or padding (3x3 stride 1 / 2): the bf6x tile
// gathers each lane's rows per (slab, tap) chunk (conv_bf6x_kernel GT)
inline bool gt_gemm(const ConvShape& s) {
  return s.Cin % CONV_BK == 0 && !(s.KH == 1 && s.KW == 1 && s.pad == 0) && s.KH * s.KW <= 32 &&
         s.has_wb && !s.has_xb;
}
// 4-channel input (NHWC4: the 7x7 stem), K order (kh, kw, c4): the bf6x tile
// gathers each lane's two taps per chunk (conv_bf6x_kernel G4)
inline bool g4_gemm(const ConvShape& s) {
  return s.Cin == 4 && s.xcs == 4 && s.KW >= 5 && s.KW <= 8 && s.has_wb && !s.has_xb &&
         s.Kpad == (s.KH * s.KW * 4 + CONV_BK - 1) / CONV_BK * CONV_BK;
}

// Split-K factor: only for deep K (>= 64 chunks) where the tile count leaves
// the last round of resident workgroups badly underfilled.
inline int choose_ksplit(long long tiles, int nch, double slots, int maxsplit) {
  // (splitting underfilled grids' shorter K too was measured no faster, r3v)
  if (nch < 64) return 1;
  int best = 1;
  double best_eff = 0.0;
  for (int ks = 1; ks <= maxsplit; ++ks) {
    if (nch / ks < 32) break;
    const double r = tiles * ks / slots;
    const double eff = r / std::ceil(r) * (ks == 1 ? 1.0 : 0.97);  // ~3% for the reduce pass
    // split only for a clear gain (A/B at 480x640: decoder layers gain nothing)
    if (eff > best_eff * 1.08) {
      best_eff = eff;
      best = ks;
    }
  }
  return best;
}

// Geometry of one tile id for this conv (ksplit = 1, no launch fields);
// kern = -1 if illegal.
inline Plan plan_for_tile(const ConvShape& s, const ConvMode& m, int tile) {
  Plan p{};
  p.kern = -1;
  p.tile = p.run_tile = tile;
  p.ksplit = 1;
  p.variant = V_NONE;
  const TileRow* r = tile_row(tile);
  if (!r) return p;
  const int fam = r->family;
  const bool cin32 = s.Cin % CONV_BK == 0;
  const bool halo_ok = cin32 && m.kmax >= KERN_HALO && s.stride == 1 && s.KH == 3 && s.KW == 3 &&
                       s.OW >= 16 && s.OH >= 8 && s.Cout % 64 == 0;
  const bool glds_ok = cin32 && m.kmax >= KERN_GLDS && s.KH * s.KW <= 32;
  const bool g4 = g4_gemm(s);
  // the convs on the bf6x tiles: 16x16x32 sums, so those tiles only, and only they
  const int xkinds = !m.bf6x_on() ? 0
                     : g4         ? XK_G4
                     : glds_ok    ? (dense_gemm(s) ? XK_DENSE : 0) | (gt_gemm(s) ? XK_GT : 0)
                                  : 0;
  const bool bf6_fam = fam == FAM_BF6 || fam == FAM_BF6B || fam == FAM_BF6R;
  // bf16x6 mode: one family group per conv -- bf6x, else fp32 halo tiles for
  // halo-eligible convs, else the bf16x6 row tiles
  if (m.bf6_on() && glds_ok) {
    if (xkinds ? fam != FAM_BF6X : fam == FAM_BF6X || (halo_ok ? fam != FAM_HALO : !bf6_fam))
      return p;
  }
  if (r->cout_div && s.Cout % r->cout_div) return p;
  switch (fam) {
    case FAM_BF6X:
      if (!(r->xkinds & (xkinds | (xkinds && !g4 && s.has_x2 ? XK_DUAL : 0)))) return p;
      p.kern = KERN_GLDS;
      break;
    case FAM_BF6B:
    case FAM_BF6R:
      if (!glds_ok || !m.bf6_on() || !s.has_wb || (r->bm == 256 && s.Cout <= 64)) return p;
      p.kern = KERN_GLDS;
      break;
    case FAM_BF6:
      if (!glds_ok || !m.bf6_on()) return p;
      p.kern = KERN_GLDS;
      break;
    case FAM_HALO:
      if (!halo_ok) return p;
      p.kern = KERN_HALO;
      // (OH >= 8 and OH * OW = hw fits an int: OW + 15 and the product do)
      p.ppi = ((s.OW + 15) / 16) * ((s.OH + r->ph - 1) / r->ph);
      break;
    default:  // FAM_ROWS, FAM_ROWS_GLDS
      // the 4-channel-input convs the G4 bf6x tile serves: it is their only
      // candidate (its sums are not bit-identical to the staged tiles')
      if (xkinds == XK_G4) return p;
      p.kern = cin32 && m.kmax >= KERN_GLDS && s.KH * s.KW <= 32 ? KERN_GLDS : KERN_STAGED;
      if (fam == FAM_ROWS_GLDS && p.kern != KERN_GLDS) {
        p.kern = -1;
        return p;
      }
      break;
  }
  p.bm = r->bm;
  p.bn = r->bn;
  p.tiles_m = p.ppi ? s.M / s.hw * p.ppi : cdiv(s.M, p.bm);
  return p;
}

// The launch of a legal plan: the A/B tile substitutions, the grid, the kernel
// instantiation and its arithmetic.
inline Plan plan_launch(const ConvShape& s, const ConvMode& m, Plan p) {
  const bool dense = dense_gemm(s);
  Plan q = p;  // geometry of the tile that runs
  if (m.bm192 && p.tile == TILE_BF6X_128x128 && p.ksplit == 1 && (dense || s.has_x2))
    q = plan_for_tile(s, m, TILE_BF6X_192x128);
  else if (m.rb4n64 && p.tile == TILE_BF6X_128x64 && p.ksplit == 1 && (dense || g4_gemm(s)) &&
           !s.has_x2)
    q = plan_for_tile(s, m, TILE_BF6X_256x64);
  if (q.kern < 0) q = p;
  const TileRow* r = tile_row(q.tile);
  p.variant = V_NONE;
  if (p.kern < 0 || !r) return p;
  p.run_tile = q.tile;
  p.threads = r->threads;
  const long long tiles_n = cdiv(s.Cout, q.bn), nwg = q.tiles_m * tiles_n;
  if (nwg * p.ksplit > INT_MAX) return p;  // grid.x
  p.tiles_n = (int)tiles_n;
  p.nwg = (int)nwg;
  p.arith = CONV_ARITH_BF6;
  const bool wide = q.bn == 128, g4 = s.Cin == 4;
  const bool unit = s.KH == 1 && s.KW == 1 && s.pad == 0;
  int v = V_NONE;
  switch (r->family) {
    case FAM_ROWS:
    case FAM_ROWS_GLDS: {
      const int v0 = q.tile == TILE_128x128  ? V_ROWS_128x128_GLDS
                     : q.tile == TILE_128x64 ? V_ROWS_128x64_GLDS
                     : q.tile == TILE_64x64  ? V_ROWS_64x64_GLDS
                                             : V_ROWS_256x128_GLDS;
      const bool stem_bf6 = q.kern != KERN_GLDS && s.Cin % CONV_BK != 0 && m.stem_bf6_on();
      v = v0 + (q.kern == KERN_GLDS ? 0 : s.Cin % CONV_BK == 0 ? 1 : stem_bf6 ? 2 : 3);
      if (!stem_bf6) p.arith = CONV_ARITH_FP32;
      break;
    }
    case FAM_HALO:
      v = q.tile == TILE_H16x128 ? V_H16x128_FP32
          : q.tile == TILE_H8x128 ? (m.halo_bf6_on() ? V_H8x128_BF6 : V_H8x128_FP32)
                                  : (m.halo_bf6_on() ? V_H8x64_BF6 : V_H8x64_FP32);
      if (v != V_H8x128_BF6 && v != V_H8x64_BF6) p.arith = CONV_ARITH_FP32;
      break;
    case FAM_BF6:
      v = q.tile == TILE_BF6_128x128   ? V_BF6_128x128
          : q.tile == TILE_BF6_128x256 ? V_BF6_128x256
          : q.tile == TILE_BF6_64x128  ? V_BF6_64x128
                                       : V_BF6_128x64;
      break;
    case FAM_BF6B:
      if (q.bm == 256)  // (its register budget caps the depth at 3)
        v = m.bf6d == 2 ? V_BF6D2_256x128 : m.bf6d ? V_BF6D3_256x128 : V_BF6B_256x128;
      else if (s.has_xb)
        v = wide ? V_BF6S_128x128 : V_BF6S_128x64;
      else if (m.bf6d && unit)  // dense: A prefetched bf6d chunks ahead in registers
        v = (wide ? V_BF6D2_128x128 : V_BF6D2_128x64) + (m.bf6d - 2);
      else
        v = wide ? V_BF6B_128x128 : V_BF6B_128x64;
      break;
    case FAM_BF6R:  // any conv, masked taps included
      v = m.bf6d ? (wide ? V_BF6D2_128x128 : V_BF6D2_128x64) + (m.bf6d - 2)
                 : (wide ? V_BF6B_128x128 : V_BF6B_128x64);
      break;
    case FAM_BF6X:
      switch (q.tile) {
        case TILE_BF6X_128x128:
          v = s.has_x2 ? V_X128_DUAL : s.has_amean ? V_X128_NORM : dense ? V_X128_DENSE : V_X128_GT;
          break;
        case TILE_BF6X_128x64: v = g4 ? V_X64_G4 : dense ? V_X64_DENSE : V_X64_GT; break;
        case TILE_BF6X_128x192: v = V_X192_DENSE; break;
        case TILE_BF6X_128x256: v = V_X256_DENSE; break;
        case TILE_BF6X_256x64: v = g4 ? V_X64_RB4_G4 : V_X64_RB4_DENSE; break;
        case TILE_BF6X_192x128: v = s.has_x2 ? V_X128_NW6_DUAL : V_X128_NW6_DENSE; break;
        default: v = dense ? V_X128_RB4_DENSE : V_X128_RB4_GT; break;  // TILE_BF6X_256x128
      }
      break;
  }
  p.variant = v;
  return p;
}
static_assert(V_BF6D4_128x128 == V_BF6D2_128x128 + 2 && V_BF6D4_128x64 == V_BF6D2_128x64 + 2 &&
                  V_ROWS_128x128_STEM_FP32 == V_ROWS_128x128_GLDS + 3,
              "plan_launch steps through CONV_VARIANTS by depth / row form");

// Default plan (heuristic), optionally overridden by a legal tile id.  The
// split factor comes from the default choice whatever the tile, and every
// tile of a conv's candidate set runs the same sums per output, so results do
// not depend on the tile (the engine's autotuner relies on this).
inline Plan conv_plan(const ConvShape& s, const ConvMode& m, bool allow_split, int forced = -1) {
  if (forced < 0 && m.tile >= 0) forced = m.tile;  // POSFEAT_CONV_TILE: any legal tile
  const bool cin32 = s.Cin % CONV_BK == 0;
  const int nch = s.Kpad / CONV_BK;
  const bool big = s.Cout > 64;
  const long long t128 = cdiv(s.M, 128) * cdiv(s.Cout, 128);
  const long long t256 = cdiv(s.M, 256) * cdiv(s.Cout, 128);
  Plan d = plan_for_tile(s, m, s.Cout % 128 == 0 ? TILE_H8x128 : TILE_H8x64);
  if (d.kern == KERN_HALO) {
    if (m.tile == TILE_H16x128 && s.Cout % 128 == 0) d = plan_for_tile(s, m, TILE_H16x128);
    const double slots = d.tile == TILE_H16x128 ? 256.0 : 512.0;
    d.ksplit = allow_split ? choose_ksplit(d.tiles_m * cdiv(s.Cout, d.bn), nch, slots,
                                           m.maxsplit)
                           : 1;
  } else {
    const int ks = (allow_split && big) ? choose_ksplit(t128, nch, 512.0, m.maxsplit) : 1;
    int tile;
    if (m.tile == TILE_256x128 && cin32 && s.Cout % 128 == 0 && t256 >= 256 && ks == 1)
      tile = TILE_256x128;
    else if (big && (t128 >= 512 || ks > 1))
      tile = TILE_128x128;
    else if (cin32 && cdiv(s.M, 128) * cdiv(s.Cout, 64) >= 512)
      tile = TILE_128x64;  // Cin = 4 layers (stem, convimg): 64x64 measured faster
    else
      tile = TILE_64x64;
    d = plan_for_tile(s, m, tile);
    d.ksplit = tile == TILE_128x128 ? ks : 1;
    if (m.bf6x_on() && g4_gemm(s)) {  // the stem: the G4 bf6x tile only
      d = plan_for_tile(s, m, TILE_BF6X_128x64);
      d.ksplit = 1;
    }
    if (m.bf6_on() && cin32 && s.KH * s.KW <= 32 && m.kmax >= KERN_GLDS) {
      const bool x = m.bf6x_on() && dense_gemm(s);
      Plan b = plan_for_tile(s, m,
                             x          ? (big ? TILE_BF6X_128x128 : TILE_BF6X_128x64)
                             : s.has_wb ? (big ? TILE_BF6B_128x128 : TILE_BF6B_128x64)
                                        : (big ? TILE_BF6_128x128 : TILE_BF6_128x64));
      if (b.kern >= 0) {
        b.ksplit = ks;
        d = b;
      }
    }
  }
  // Cin % 32 convs with taps on the pre-split planes: the GT bf6x tile
  if (m.bf6x_on() && gt_gemm(s) && m.kmax >= KERN_GLDS) {
    Plan b = plan_for_tile(s, m, big ? TILE_BF6X_128x128 : TILE_BF6X_128x64);
    if (b.kern >= 0) {
      b.ksplit = allow_split ? choose_ksplit(t128, nch, 768.0, m.maxsplit) : 1;
      d = b;
    }
  }
  if (forced >= 0) {
    Plan f = plan_for_tile(s, m, forced);
    if (f.kern >= 0) {
      f.ksplit = d.ksplit;
      d = f;
    }
  }
  return plan_launch(s, m, d);
}

// pf_gemm_batched (nb GEMMs [M][K] x [N][K]^T in one grid): the tile to force,
// -1 for conv_plan's own choice.  The heuristic sizes tiles for ONE GEMM; with
// nb of them in the grid the 128x128 tile still fills the chip.  N = 192
// (head.conv1's Winograd GEMMs): one 192-wide column tile reads A once.
inline int gemm_batched_tile(long long M, int N, int nb, bool has_Bb, const ConvMode& m) {
  // (tiles of all nb GEMMs >= 1024, the count capped so the product fits)
  const bool fills = cdiv(M, 128) * cdiv(N, 128) * (nb < 1024 ? nb : 1024) >= 1024;
  if (has_Bb && m.bf6x_on())
    return m.n256 && N % 256 == 0 ? TILE_BF6X_128x256
           : N % 128 == 0         ? (m.rb4 ? TILE_BF6X_256x128 : TILE_BF6X_128x128)
           : N % 192 == 0         ? TILE_BF6X_128x192
                                  : TILE_BF6X_128x64;
  return (has_Bb && m.gemm_b256 && N % 128 == 0)  ? TILE_BF6B_256x128
         : (N % 128 == 0 && fills)                ? TILE_128x128
         : (has_Bb && N % 128 != 0 && N % 64 == 0) ? TILE_BF6B_128x64
                                                   : -1;
}
// ... and whether the weight-stationary batched kernel is asked first (the
// short-K Winograd GEMMs: head.conv1's K = 192, layer2's 128, layer3's 256)
inline bool gemm_batched_ws_first(int K, bool has_Bb, const ConvMode& m) {
  return m.wsb && has_Bb && m.bf6x_on() &&
         (K == 192 || (K == 128 && m.wsb >= 2) || (K == 256 && m.wsb >= 3));
}
