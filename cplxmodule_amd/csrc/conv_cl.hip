// Complex 3 x 3 convolution (stride 1, "same" zero padding) on UNPADDED channels-last activations, bf16 in / bf16
// out, fp32 accumulation: forward and data gradient of cplx.conv2d (cplxmodule/cplx.py:770-838) for the shapes of
// BASELINE cfg3 / cfg5.  Round-2 rebuild of conv_nhwc.hip along the lines of profiles/r01_conv_ablation.md, with
// what the persistent GEMM (gemm_bf16_persist.h) taught:
//
//  * activations stay channels-last end to end: x[P][C], y[P][Cout] with P = B H W (torch.channels_last storage of
//    the usual [B, C, H, W] tensors).  No padded grid, no pad passes, no transpose in the epilogue: a tap is a row
//    shift `x[p + (kh d - ph) W + (kw d - pw)]`, and the rows a shift drags in from the neighbouring image row /
//    image are masked when the A fragment is read -- by ADDRESS: a masked lane reads a 16-byte row of zeros kept in
//    LDS, one v_bfi per fragment instead of four selects on its data.  Rows before / after the tensor are never
//    fetched: the LDS-DMA is `buffer_load_dwordx4 ... offen lds`, whose range check writes zeros for them
//    (probe: scripts/r02/bufload_oob.hip).
//  * implicit GEMM [512 pixels] x [64 output channels] per workgroup of 8 waves (64 x 64 complex per wave = 128
//    accumulators), K = KH x C/16 stages of (kernel row, 16 input channels) x KW taps; a stage stages 512 input
//    rows ONCE for the KW taps of its kernel row (an output tile is 512 - (KW-1) d pixels; neighbouring tiles
//    overlap by the halo) plus that stage's weights: EVERYTHING in the K loop arrives by LDS-DMA, so the counted
//    s_waitcnt vmcnt is exact (the r01 kernel mixed LDS-DMA with register weight loads and lost its prefetch
//    distance to the in-order counter).  44 KiB per stage, 3-slot ring.
//  * persistent: one workgroup per CU walks its tiles (XCD-contiguous ranges), the ring runs through the tile
//    boundary, the epilogue stages rows through LDS above the ring and writes whole 128-byte lines; the next
//    tile's bias arrives by one more LDS-DMA.  Same boundary schedule as the GEMM: the last stage issues the whole
//    third stage of the next tile BEFORE the stores, and nothing issued after the stores is waited for until two
//    stages later.
//  * weights are pre-packed per (output-channel tile, stage) as the LDS image itself (csrc: pack_kernel), with
//    the conjugate / flip / channel swap of the data gradient folded into the packing, so the kernel has one form.
//
// The same source is the REAL-valued kernel (CPLX = false): the variance path of the local-reparameterization
// convolution layers (conv of |x|^2 with exp(log_sigma2), cplxmodule/nn/relevance/complex/base.py:120-135,
// real/base.py:116-163) and the real Conv2dVD / ARD layers.  Everything the two variants differ in is derived from
// CPLX in Geo below; the kernel, the packing and the launcher are written once in those terms.
#include <type_traits>

#include "common.h"
#include "prims.h"
#include "launch.h"   // per-call launch policy (CPLXAMD_LAUNCH_SHARED: the chip is shared with collectives)

namespace cplxamd {
namespace cl {

constexpr int NT = 512, BN = 64;
constexpr int NST = 16;                       // global stores per wave in the epilogue (NP planes x IB blocks x 4 rounds)

// What the complex and the real kernel differ in.  A complex block pair costs four MFMAs (re/im x re/im), a real one
// a single MFMA, so the real wave takes twice the pixels for the same 128 accumulators and the same MFMAs per byte
// staged: complex 2 planes x (2 x 2) blocks per wave, workgroup tile 512 grid pixels, 44 KiB per stage for 192 MFMAs per
// wave; real 1 plane x (4 x 2) blocks, 1024 grid pixels, 38 KiB per stage for 96.
template <int KW, bool CPLX> struct Geo {
  static constexpr int NP = CPLX ? 2 : 1;                      // planes of every operand
  static constexpr int IB = CPLX ? 2 : 4;                      // 32-pixel blocks per wave (x 2 blocks of 32 channels)
  static constexpr int TM = 8 * 32 * IB;                       // grid pixels per workgroup tile (8 waves)
  static constexpr int A_PLANE = TM * 32 + 64;                 // TM rows x 16 channels, then the zero row (row TM)
  static constexpr int ZROW = TM * 32;                         // plane-relative byte address of the zero row
  static constexpr int AP = TM * 32 / 8192;                    // LDS-DMA pieces (8 KiB per workgroup) of one A plane
  static constexpr int NA = NP * AP;                           // ... of the activations: 4 either way
  static constexpr int W_PLANE = KW * 64 * 32;                 // [kw][64 co][16 ch] bf16
  static constexpr int W_BYTES = NP * W_PLANE;
  static constexpr int STAGE = NP * A_PLANE + W_BYTES;
  static constexpr int PWN = (W_BYTES + 8191) / 8192;          // LDS-DMA pieces of the weights
  static constexpr int W_BACK = W_BYTES / 16 < NT ? W_BYTES / 16 : NT;   // surplus lanes of the last weight piece re-read
                                                               // the chunk this far back (a piece, or the whole image
                                                               // when that is shorter) into the dump
  static constexpr int L = NA + PWN;                           // pieces per stage and wave
  static constexpr int GRP = IB * 2;                           // block pairs = MFMA groups per tap
  static constexpr int MPG = NP * NP;                          // MFMAs per group
  static constexpr int NRD = NP * (2 + IB);                    // fragment reads per tap: NP x (2 weight + IB activation)
  static constexpr int RPG = (NRD + GRP - 1) / GRP;            // ... per group: 8 over 4 groups / 6 over the first 6 of 8
  static constexpr int EPI = 3 * STAGE;                        // per wave: 16 epilogue rows of 144 B, then 512 B of bias
  static constexpr int EPI_WAVE = 16 * 144 + 512;
  static constexpr int DUMP = EPI + 8 * EPI_WAVE;              // where the surplus half of a weight piece goes
  static constexpr int SMEM = DUMP + 4096;
};

template <bool CPLX> struct Args {
  static constexpr int NP = CPLX ? 2 : 1;    // planes: real, imaginary
  const void* x[NP];                         // [P][C] bf16
  const void* w;                             // packed weights (pack_kernel)
  const float* bias[NP];                     // [Cout] or null
  void* y[NP];                               // [P][Cout] bf16
  void* dump;                                // TM x Cout bf16: where the rows a tile does not own are stored
  int64_t P;
  uint32_t x_bytes, w_bytes;                 // bytes of one activation plane / of the packed weights
  int H, W, C, Cout, KH, dil_h, dil_w, pad_h, pad_w;   // H x W: the grid the tiles walk (the larger of the two images)
  int Hi, Wi, Ho, Wo;                        // extent of the input / output image, both top-left aligned on that grid
  int C16, NS, tm_out, tiles_m, tiles_n;
  FastDiv div_w, div_h;
  int stagger, stagger_from;                 // start delay: (blockIdx - stagger_from) * stagger clocks (0 below stagger_from)
};

enum { FL_NORMAL = 0, FL_FIRST0 = 1, FL_LAST = 2, FL_FIRST1 = 3 };

template <int KW, bool CPLX>
__global__ __launch_bounds__(NT) void conv_cl_kernel(Args<CPLX> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using G = Geo<KW, CPLX>;
  constexpr int L = G::L, STAGE = G::STAGE, NP = G::NP, IB = G::IB, AP = G::AP, A_PLANE = G::A_PLANE, ZROW = G::ZROW;
  static_assert(L + NST <= 63, "vmcnt is a 6-bit counter");

  const int ntiles = g.tiles_m * g.tiles_n;
  const int nwg = gridDim.x;
  // virtual block id -> tile (XCD x owns a contiguous range of the tile order; consecutive tiles of the order
  // share their halo rows and, across column tiles, their whole input window)
  auto origin = [&](int v, int& r0, int& nt_) __attribute__((always_inline)) {
    const int q = ntiles >> 3, r = ntiles & 7, xcd = v & 7, idx = v >> 3;
    const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = lin / g.tiles_n;
    nt_ = __builtin_amdgcn_readfirstlane(lin - mt * g.tiles_n);
    r0 = __builtin_amdgcn_readfirstlane(mt * g.tm_out);
  };

  const int tid0 = threadIdx.x;
  const int lane = tid0 & 63, wid = tid0 >> 6;
  const int l31 = lane & 31, lk = lane >> 5;
  const int wm = wid * 32 * IB;

  // zero rows, 16 dwords per slot and plane (never overwritten: the A pieces cover rows 0..TM-1 exactly)
  if (tid0 < 3 * NP * 16) {
    const int slot = tid0 / (NP * 16), r = tid0 % (NP * 16);
    *reinterpret_cast<uint32_t*>(smem + slot * STAGE + (r >> 4) * A_PLANE + ZROW + (r & 15) * 4) = 0u;
  }

  // (the plane arrays of Args are read at constant indices only: a subscript that is a loop counter, even of an unrolled
  //  loop, keeps the whole argument block from being split into scalars up front)
  const i32x4 rs_xr = make_rsrc(g.x[0], g.x_bytes), rs_xi = make_rsrc(g.x[NP - 1], g.x_bytes);
  const i32x4 rs_w = make_rsrc(g.w, g.w_bytes);
  const uint32_t rowbytes = (uint32_t)g.C * 2u;

  const uint32_t smem_off = lds_offset_of(smem);
  const uint32_t wid_u = (uint32_t)__builtin_amdgcn_readfirstlane(tid0 >> 6);
  const uint32_t wave_lds = wid_u * 1024u;

  // per-lane source offsets of the LDS-DMA pieces.  A plane: chunk p = j*512 + tid sits at LDS row p >> 1, position
  // p & 1, and holds channel half (p & 1) ^ ((row >> 3) & 1) of input row `row` of the window (so that the 16 lanes
  // of a ds_read_b128 group hit 16 distinct 16-byte bank groups).  Weights: the packed stage IS the LDS image.
  uint32_t voa[AP], vow[G::PWN];
#pragma unroll
  for (int j = 0; j < AP; ++j) {
    const int p = j * NT + tid0, row = p >> 1, c = (p & 1) ^ ((row >> 3) & 1);
    voa[j] = (uint32_t)row * rowbytes + (uint32_t)c * 16u;
  }
#pragma unroll
  for (int j = 0; j < G::PWN; ++j) {
    int p = j * NT + tid0;
    if (p >= G::W_BYTES / 16) p -= G::W_BACK;              // surplus lanes re-read valid chunks into the dump
    vow[j] = (uint32_t)p * 16u;
  }

  // An input image smaller than the grid (the data gradient of a convolution with less than `same` padding reads the
  // (Ho, Wo) output gradient on the (H, W) grid of the input): a window row is a grid pixel, its source the pixel of the
  // same coordinates in the dense input -- no longer window start + row, so the lane offsets are rebuilt per tile
  // (two divisions per piece).  Pixels outside the input alias others or fall out of range; the fragment masks skip them.
  const bool in_dense = g.Hi == g.H && g.Wi == g.W;
  uint32_t voa_c[AP], voa_n[AP];                   // offsets of the tile the LDS-DMA pointer is in / of the one after it
  auto lane_offsets = [&](int rr, uint32_t (&out)[AP]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < AP; ++j) {
      if (in_dense) { out[j] = voa[j]; continue; }
      const int pr = j * NT + tid0, row = pr >> 1, c = (pr & 1) ^ ((row >> 3) & 1);
      // (the kernel-row part of the shift stays in the scalar offset: it may turn a row that starts above the image,
      //  i.e. at a wrapped "negative" offset, into a valid one two kernel rows later)
      const int64_t pix = (int64_t)rr - g.pad_w + row;
      uint32_t o = 0xF8000000u;
      if (pix >= 0 && pix < g.P) {
        const uint32_t q = (uint32_t)pix, qh = fast_div(q, g.div_w), w = q - qh * (uint32_t)g.W;
        const uint32_t b = fast_div(qh, g.div_h), h = qh - b * (uint32_t)g.H;
        o = ((b * (uint32_t)g.Hi + h) * (uint32_t)g.Wi + w) * rowbytes + (uint32_t)c * 16u;
      }
      out[j] = o;
    }
  };

  // fragment addresses relative to the slot.  x: row = wm + i*32 + l31 + kw*dil_w; w: co = j*32 + l31.
  uint32_t a_rel[IB][KW], w_rel[2];
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      const int row = wm + i * 32 + l31 + kw * g.dil_w;
      a_rel[i][kw] = (uint32_t)(row * 32 + ((lk ^ ((row >> 3) & 1)) << 4));
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = j * 32 + l31;
    w_rel[j] = (uint32_t)(NP * A_PLANE + co * 32 + ((lk ^ ((co >> 3) & 1)) << 4));
  }

  // (one array per plane, not [NP]: the imaginary ones are simply never touched by the real kernel and vanish)
  f32x16 acc_r[IB][2], acc_i[IB][2];                       // [pixel block][channel block]
  bf16x8 ar[2][IB], ai[2][IB], br[2][2], bi[2][2];         // [set][block]

  // ---- tiles -------------------------------------------------------------------------------------------------
  int v = blockIdx.x;
  int r0, nt0, r0n, ntn;
  origin(v, r0, nt0);
  bool has_next = v + nwg < ntiles;
  origin(has_next ? v + nwg : v, r0n, ntn);

  // ---- the LDS-DMA stage pointer: runs three stages ahead of the MFMAs, through the tile boundaries ----------
  const uint32_t kh_step = (uint32_t)(g.dil_h * g.Wi) * rowbytes - (uint32_t)(g.C16 - 1) * 32u;
  auto a_origin = [&](int rr) __attribute__((always_inline)) -> uint32_t {
    // window of kernel row 0 starts pad_h image rows and pad_w pixels before the tile (wraps below zero: out of range)
    return in_dense ? (uint32_t)(rr - g.pad_w - g.pad_h * g.W) * rowbytes : (uint32_t)(-g.pad_h * g.Wi) * rowbytes;
  };
  lane_offsets(r0, voa_c);
  lane_offsets(r0n, voa_n);
  uint32_t d_aoff = a_origin(r0), d_woff = (uint32_t)(nt0 * g.NS) * (uint32_t)G::W_BYTES;
  int d_cs = 0, d_u = 0;
  auto dma_advance = [&]() __attribute__((always_inline)) {
    ++d_u; ++d_cs;
    d_woff += (uint32_t)G::W_BYTES;
    if (d_cs == g.C16) { d_cs = 0; d_aoff += kh_step; } else { d_aoff += 32u; }
    if (d_u == g.NS) {                                     // on to the next tile of this workgroup (or this one again)
      d_u = 0; d_cs = 0;
      d_aoff = a_origin(r0n);
      d_woff = (uint32_t)(ntn * g.NS) * (uint32_t)G::W_BYTES;
#pragma unroll
      for (int j = 0; j < AP; ++j) voa_c[j] = voa_n[j];
    }
  };
  const uint32_t soff[3] = {smem_off, smem_off + (uint32_t)STAGE, smem_off + 2u * (uint32_t)STAGE};
  // piece q of the stage at the pointer -> slot
  auto dma_piece = [&](int q, uint32_t slot_off) __attribute__((always_inline)) {
    // AP pieces of the real plane, (CPLX) AP of the imaginary one, then the weights
    if (q < AP) buf_lds16_soff(rs_xr, voa_c[q] + d_aoff, 0u, slot_off + (uint32_t)(q * 8192) + wave_lds);
    else if (q < G::NA)
      buf_lds16_soff(rs_xi, voa_c[q - AP] + d_aoff, 0u, slot_off + (uint32_t)(A_PLANE + (q - AP) * 8192) + wave_lds);
    else {
      const int j = q - G::NA;
      constexpr int FULLW = G::W_BYTES / 1024;             // waves of weight data in total
      const bool real = (uint32_t)(j * 8) + wid_u < (uint32_t)FULLW;
      const uint32_t dst = real ? slot_off + (uint32_t)(NP * A_PLANE + j * 8192) + wave_lds
                                : smem_off + (uint32_t)G::DUMP + (wave_lds & 4095u);
      buf_lds16_soff(rs_w, vow[j], d_woff, dst);
    }
  };

  // ---- masks: bit kw = column tap kw stays inside the image row, bit 8 + kh = row tap kh stays inside the image
  uint32_t vmask[IB];
  auto tile_masks = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      const uint32_t q = (uint32_t)(r0 + wm + i * 32 + l31);
      const uint32_t qh = fast_div(q, g.div_w), w = q - qh * (uint32_t)g.W;
      const uint32_t h = qh - fast_div(qh, g.div_h) * (uint32_t)g.H;
      uint32_t m = 0;
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) {
        const int ww = (int)w + kw * g.dil_w - g.pad_w;
        m |= (ww >= 0 && ww < g.Wi) ? (1u << kw) : 0u;
      }
      for (int kh = 0; kh < g.KH; ++kh) {
        const int hh = (int)h + kh * g.dil_h - g.pad_h;
        m |= (hh >= 0 && hh < g.Hi) ? (0x100u << kh) : 0u;
      }
      vmask[i] = m;
    }
  };
  int c_kh = 0, c_cs = 0;                                  // (kernel row, channel slice) of the stage the MFMAs are in
  auto masked = [&](int i, int kw, int kh) __attribute__((always_inline)) -> uint32_t {
    const uint32_t hb = (vmask[i] >> (8 + kh)) & 1u;
    const uint32_t sel = (0u - hb) & vmask[i];
    const uint32_t m = (uint32_t)((int32_t)(sel << (31 - kw)) >> 31);
    return (a_rel[i][kw] & m) | ((uint32_t)ZROW & ~m);
  };

  // fragment idx of tap kw of the stage in slot `sl` -> register set `st`: the NP planes of the fragments in the order
  // w 0, x 0, w 1, x 1, (x 2, x 3) -- what the first MFMA groups need first
  auto read_one = [&](int st, const char* sl, int kw, int kh, int idx) __attribute__((always_inline)) {
    const int f = idx / NP;
    const bool im = idx % NP;
    const char* wr_ = sl + kw * 2048;
    const char* wi_ = wr_ + G::W_PLANE;
    if (f == 0 || f == 2) {
      if (!im) br[st][f >> 1] = *reinterpret_cast<const bf16x8*>(wr_ + w_rel[f >> 1]);
      else bi[st][f >> 1] = *reinterpret_cast<const bf16x8*>(wi_ + w_rel[f >> 1]);
    } else {
      const int i = f == 1 ? 0 : f - 2;
      if (!im) ar[st][i] = *reinterpret_cast<const bf16x8*>(sl + masked(i, kw, kh));
      else ai[st][i] = *reinterpret_cast<const bf16x8*>(sl + A_PLANE + masked(i, kw, kh));
    }
  };

  // GRP groups of MPG MFMAs on register set `st`; behind group n its RPG fragment reads of (slot rsl, tap rkw, kernel
  // row rkh) into the other set (NRD in all) and the LDS-DMA pieces [q0, q1) of the stage at the pointer -> slot ds,
  // spread over the groups
  auto mfma_sub = [&](int st, const char* rsl, int rkw, int rkh, bool do_read, uint32_t ds, int q0, int q1)
      __attribute__((always_inline)) {
    bf16x8 nai[IB];
    int q = q0;
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (CPLX) {
          if (j == 0) nai[i] = neg_frag(ai[st][i]);        // (not earlier: block 1's fragments were read last)
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(br[st][j], ar[st][i], acc_r[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(br[st][j], ai[st][i], acc_i[i][j], 0, 0, 0);
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bi[st][j], nai[i], acc_r[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bi[st][j], ar[st][i], acc_i[i][j], 0, 0, 0);
        } else {
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(br[st][j], ar[st][i], acc_r[i][j], 0, 0, 0);
        }
        const int grp = i * 2 + j;
        __builtin_amdgcn_sched_barrier(0);
        if (do_read) {
#pragma unroll
          for (int r = 0; r < G::RPG; ++r)
            if (G::RPG * grp + r < G::NRD) read_one(st ^ 1, rsl, rkw, rkh, G::RPG * grp + r);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int left = G::GRP - grp;
        const int n_now = (q1 - q + left - 1) / left;
#pragma unroll
        for (int r = 0; r < 6; ++r)
          if (r < n_now && q < q1) {
            __builtin_amdgcn_sched_barrier(0);
            dma_piece(q, ds);
            __builtin_amdgcn_sched_barrier(0);
            ++q;
          }
      }
  };

  const char* const sbase[3] = {smem, smem + STAGE, smem + 2 * STAGE};

  // one stage: tap 0 | tap 1 | [all reads of this slot done, next stage landed: barrier] | tap 2.
  // LDS-DMA: pieces 2.. of the stage two ahead (-> the slot the previous stage left) behind taps 0 and 1, pieces 0, 1
  // of the stage three ahead (-> this stage's slot) behind tap 2.  PAR = register set holding (this stage, tap 0).
  auto body = [&](auto SLOT, auto PARITY, auto FLAVOUR) __attribute__((always_inline)) {
    constexpr int kc = decltype(SLOT)::value, par = decltype(PARITY)::value, fl = decltype(FLAVOUR)::value;
    static_assert(KW == 3, "the tap schedule below is written for three taps");
    const uint32_t o0 = soff[kc], o2 = soff[(kc + 2) % 3];
    const char* p0 = sbase[kc];
    const char* p1 = sbase[(kc + 1) % 3];
    const int kh = c_kh;
    if (fl == FL_FIRST0) {                                 // the stage two ahead was issued whole before the stores
      mfma_sub(par, p0, 1, kh, true, o2, 0, 0);
      mfma_sub(par ^ 1, p0, 2, kh, true, o2, 0, 0);
    } else {
      mfma_sub(par, p0, 1, kh, true, o2, 2, G::NA);
      mfma_sub(par ^ 1, p0, 2, kh, true, o2, G::NA, L);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // (FIRST0 / FIRST1: the stages they need landed before the stores' wait; a plain vmcnt(L) would wait for the
    //  epilogue's stores, which are older than the pieces issued since)
    if (fl == FL_FIRST1) wait_vmcnt<L + NST>();
    else if (fl != FL_FIRST0) wait_vmcnt<L>();
    __builtin_amdgcn_s_barrier();
    // the MFMAs move on to the next stage
    if (++c_cs == g.C16) { c_cs = 0; ++c_kh; }
    dma_advance();
    if (fl == FL_LAST) mfma_sub(par, p1, 0, 0, false, o0, 0, L);   // whole next-tile stage 2; its first fragments are
    else mfma_sub(par, p1, 0, c_kh, true, o0, 0, 2);               // read after the epilogue (32 registers less there)
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;

  // thread id the compiler cannot see through: addresses of per-tile code are rebuilt from it instead of being
  // hoisted across the K loop (where they would be spilled, and a scratch reload behind the stores waits for them)
  auto opaque_tid = [&]() __attribute__((always_inline)) -> int {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  };

  // ---- epilogue: 8 rows x 128 bytes per round through this wave's 2 KiB; NST unpredicated stores per wave (rows a
  // tile does not own -- the overlap with the next tile, rows past the tensor -- go to the dump buffer)
  auto epilogue = [&](int nt_) __attribute__((always_inline)) {
    const int t = opaque_tid();
    const int ln = t & 63, w_ = t >> 6, q31 = ln & 31, qk = ln >> 5;
    const int wm_ = w_ * 32 * IB;
    char* reg = smem + G::EPI + w_ * G::EPI_WAVE;
    constexpr int PITCH = 144;
    const int r16 = q31 >> 4, rr = q31 & 15;
    const int64_t ldc = g.Cout;
    const bool out_dense = g.Ho == g.H && g.Wo == g.W, wide = g.W >= 32 * IB;
    uint32_t w_first = 0, h_first = 0, b_first = 0;       // grid coordinates of this lane's first row (r0 + wm + lane / 8)
    if (!out_dense) {
      const uint32_t q = (uint32_t)(r0 + wm_ + (ln >> 3)), qh = fast_div(q, g.div_w);
      w_first = q - qh * (uint32_t)g.W; b_first = fast_div(qh, g.div_h); h_first = qh - b_first * (uint32_t)g.H;
    }
    int64_t own = g.P - r0;
    if (own > g.tm_out) own = g.tm_out;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
      bf16_t* out = reinterpret_cast<bf16_t*>(pl ? g.y[NP - 1] : g.y[0]);
#pragma unroll
      for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          if (r16 == half) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                f4 x;
#pragma unroll
                for (int e = 0; e < 4; ++e) x.v[e] = pl ? acc_i[i][j][4 * q + e] : acc_r[i][j][4 * q + e];
                st4(reinterpret_cast<bf16_t*>(reg + rr * PITCH + (j * 32 + 8 * q + 4 * qk) * 2), x);
              }
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int sub = 0; sub < 2; ++sub) {
            const uint4 val = *reinterpret_cast<const uint4*>(reg + (sub * 8 + (ln >> 3)) * PITCH + (ln & 7) * 16);
            const int m = wm_ + i * 32 + half * 16 + sub * 8 + (ln >> 3);
            const int col = nt_ * BN + (ln & 7) * 8;
            int64_t orow = (int64_t)r0 + m;
            bool ok = m < own;
            if (!out_dense) {                       // output image smaller than the grid: its own dense row index
              uint32_t w = w_first + (uint32_t)(i * 32 + half * 16 + sub * 8), h = h_first, b = b_first;
              if (wide) {                           // (one carry at most for the 32 IB rows of a wave)
                if (w >= (uint32_t)g.W) { w -= (uint32_t)g.W; if (++h == (uint32_t)g.H) { h = 0; ++b; } }
              } else {
                const uint32_t q = (uint32_t)orow, qh = fast_div(q, g.div_w);
                w = q - qh * (uint32_t)g.W; b = fast_div(qh, g.div_h); h = qh - b * (uint32_t)g.H;
              }
              ok = ok && h < (uint32_t)g.Ho && w < (uint32_t)g.Wo;
              orow = ((int64_t)b * g.Ho + h) * g.Wo + w;
            }
            bf16_t* dst = ok ? out + orow * ldc + col : reinterpret_cast<bf16_t*>(g.dump) + (int64_t)m * ldc + col;
            // streaming stores: the output is read by a later kernel, not by this one (-1.4 %)
            typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(u32x4_t{val.x, val.y, val.z, val.w}, reinterpret_cast<u32x4_t*>(dst));
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
  };

  // bias of column tile nt_ -> this wave's 512 bytes behind its epilogue rows (16 lanes per plane)
  const uint32_t bias_lds = smem_off + (uint32_t)G::EPI + wid_u * (uint32_t)G::EPI_WAVE + 2304u;
  auto bias_dma = [&](int nt_) __attribute__((always_inline)) {
    const int t = opaque_tid();
    const int ln = t & 63;
    if (ln < 16 * NP) {
      const float* src = g.bias[0] ? (CPLX ? (ln < 16 ? g.bias[0] : g.bias[NP - 1]) + nt_ * BN + 4 * (ln & 15)
                                           : g.bias[0] + nt_ * BN + 4 * ln)
                                   : reinterpret_cast<const float*>(g.w) + 4 * ln;
      lds_dma16_at(src, bias_lds);
    }
  };
  auto init_acc = [&]() __attribute__((always_inline)) {
    const int t = opaque_tid();
    const int w_ = t >> 6, qk = (t & 63) >> 5;
    const char* breg = smem + G::EPI + w_ * G::EPI_WAVE + 2304;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f4 bv = {{0.f, 0.f, 0.f, 0.f}};
          if (g.bias[0]) bv = ld4(reinterpret_cast<const float*>(breg + pl * 256 + (j * 32 + 8 * q + 4 * qk) * 4));
#pragma unroll
          for (int i = 0; i < IB; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (pl) acc_i[i][j][4 * q + e] = bv.v[e];
              else acc_r[i][j][4 * q + e] = bv.v[e];
            }
        }
  };
  auto first_frags = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int idx = 0; idx < G::NRD; ++idx) read_one(0, sbase[0], 0, 0, idx);
  };

  // start stagger: tiles take the same time on every CU, so without it all 256 CUs reach their epilogues together
  // and the 128 KiB per CU of stores arrive at the L2s / HBM as one burst per tile
  {
    const int n = __builtin_amdgcn_readfirstlane(((int)blockIdx.x - g.stagger_from) * g.stagger);
    for (int i = 0; i < n; i += 32 * 64) __builtin_amdgcn_s_sleep(32);
  }
  // ---- prologue of the first tile: stages 0, 1, 2 whole (the state every later tile starts from) -------------
  __syncthreads();                                         // zero rows written
  bias_dma(nt0);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int q = 0; q < L; ++q) dma_piece(q, soff[s]);
    if (s < 2) dma_advance();
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  init_acc();
  tile_masks();
  first_frags();

  const int npairs = (g.NS - 6) / 6;
  for (;;) {
    c_kh = 0; c_cs = 0;
    body(I0{}, I0{}, I1{});                                // FIRST0
    body(I1{}, I1{}, I3{});                                // FIRST1
    body(I2{}, I0{}, I0{});
    for (int pr = 0; pr < npairs; ++pr) {
      body(I0{}, I1{}, I0{}); body(I1{}, I0{}, I0{}); body(I2{}, I1{}, I0{});
      body(I0{}, I0{}, I0{}); body(I1{}, I1{}, I0{}); body(I2{}, I0{}, I0{});
    }
    body(I0{}, I1{}, I0{});
    body(I1{}, I0{}, I0{});
    body(I2{}, I1{}, I2{});                                // LAST
    bias_dma(has_next ? ntn : nt0);                        // (older than the stores below)
    epilogue(nt0);
    if (!has_next) break;
    wait_vmcnt<NST>();                                     // everything issued BEFORE the stores has landed
    v += nwg;
    r0 = r0n; nt0 = ntn;
    has_next = v + nwg < ntiles;
    origin(has_next ? v + nwg : v, r0n, ntn);
    lane_offsets(r0n, voa_n);
    init_acc();
    tile_masks();
    first_frags();
  }
  wait_vmcnt<0>();                                         // surplus pieces of the last tail land before the LDS is released
}

// ---- weight packing: [Co][Ci][KH][KW] planes (bf16) -> per (column tile, kernel row, 16-channel slice) the LDS image
// [plane][kw][64 n][2 chunk positions][8] with chunk position cp holding channel half cp ^ ((n >> 3) & 1).
// dgrad: n runs over Ci, the contraction over Co, both kernel axes flipped, imaginary plane negated (conj).
// (w_i: unused by the real kernel)
template <bool CPLX>
__global__ void pack_kernel(const bf16_t* w_r, const bf16_t* w_i, bf16_t* out, int Co, int Ci, int KH, int KW, int dgrad,
                            int64_t total) {
  const int N = dgrad ? Ci : Co, C = dgrad ? Co : Ci;
  const int C16 = C / 16;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = o;
    const int e = (int)(t & 7); t >>= 3;
    const int cp = (int)(t & 1); t >>= 1;
    const int nl = (int)(t & 63); t >>= 6;
    const int kw = (int)(t % KW); t /= KW;
    int pl = 0;
    if constexpr (CPLX) { pl = (int)(t & 1); t >>= 1; }
    const int cs = (int)(t % C16); t /= C16;
    const int kh = (int)(t % KH); t /= KH;
    const int nt = (int)t;
    const int n = nt * 64 + nl;
    const int c = cs * 16 + ((cp ^ ((nl >> 3) & 1)) << 3) + e;
    bf16_t val = 0;
    if (n < N) {
      const bf16_t* src = CPLX && pl ? w_i : w_r;
      if (!dgrad) val = src[(((int64_t)n * Ci + c) * KH + kh) * KW + kw];
      else {
        val = src[(((int64_t)c * Ci + n) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)];
        if constexpr (CPLX)
          if (pl) val ^= 0x8000u;
      }
    }
    out[o] = val;
  }
}

// channels-last [B][S][C] -> planar [B][C][S] (bf16), 64 pixels x 64 channels per block through LDS: the way back for
// a caller that holds plain contiguous tensors (a gradient for an NCHW leaf); 16-byte accesses on both sides.
__global__ __launch_bounds__(256) void cl_to_nchw_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int C,
                                                         int64_t S) {
  __shared__ bf16_t tile[64][64 + 8];                        // [pixel][channel]
  const int ctiles = (C + 63) / 64;
  const int64_t b = blockIdx.y / ctiles;
  const int c0 = (int)(blockIdx.y - b * ctiles) * 64;
  const int64_t s0 = (int64_t)blockIdx.x * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int idx = r * 256 + tid, p = idx >> 3, c8 = (idx & 7) * 8;
    uint4 v = uint4{0, 0, 0, 0};
    if (s0 + p < S && c0 + c8 < C) v = *reinterpret_cast<const uint4*>(x + ((int64_t)b * S + s0 + p) * C + c0 + c8);
    *reinterpret_cast<uint4*>(&tile[p][c8]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int idx = r * 256 + tid, c = idx >> 3, p8 = (idx & 7) * 8;
    if (c0 + c >= C || s0 + p8 >= S) continue;
    bf16_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[p8 + e][c];
    *reinterpret_cast<uint4*>(out + ((int64_t)b * C + c0 + c) * S + s0 + p8) = *reinterpret_cast<const uint4*>(v);
  }
}

}  // namespace cl
}  // namespace cplxamd

using namespace cplxamd;

// ---- the complex (cl) and the real (clr) entry points: one body each, instantiated twice --------------------------

template <bool CPLX> static int64_t cl_pack_bytes(int N, int C, int KH, int KW) {
  if (N <= 0 || C <= 0 || KH <= 0 || KW <= 0 || C % 16) return 0;
  return (int64_t)((N + 63) / 64) * KH * (C / 16) * (CPLX ? 2 : 1) * KW * 64 * 16 * 2;
}
template <bool CPLX> static int64_t cl_ws_bytes(int Cout) {
  return Cout > 0 ? (int64_t)cl::Geo<3, CPLX>::TM * Cout * 2 : 0;
}

template <bool CPLX>
static int cl_pack(const void* w_r, const void* w_i, void* out, int Co, int Ci, int KH, int KW, int dgrad, void* stream) {
  if (!w_r || (CPLX && !w_i) || !out || Co <= 0 || Ci <= 0 || KH <= 0 || KW <= 0) return CPLXAMD_EINVAL;
  if ((dgrad ? Co : Ci) % 16) return CPLXAMD_ESHAPE;
  const int64_t total = cl_pack_bytes<CPLX>(dgrad ? Ci : Co, dgrad ? Co : Ci, KH, KW) / 2;
  cl::pack_kernel<CPLX><<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(
      (const bf16_t*)w_r, (const bf16_t*)w_i, (bf16_t*)out, Co, Ci, KH, KW, dgrad, total);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

// x, bias, y: the real plane, then (CPLX) the imaginary one
template <bool CPLX>
static int cl_launch(const void* const (&x)[2], const void* w_packed, const float* const (&bias)[2], void* const (&y)[2],
                     int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, int mode,
                     void* ws, int64_t ws_bytes, int flags, void* stream) {
  using G3 = cl::Geo<3, CPLX>;
  constexpr int NP = G3::NP, TM = G3::TM;
  if (!launch_flags_ok(flags)) return CPLXAMD_EINVAL;
  if (!w_packed || B < 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || KH <= 0 || KW <= 0 || dil_h <= 0 || dil_w <= 0 ||
      pad_h < 0 || pad_w < 0 || (mode != 0 && mode != 1))
    return CPLXAMD_EINVAL;
  for (int pl = 0; pl < NP; ++pl)
    if (!x[pl] || !y[pl] || (bias[pl] == nullptr) != (bias[0] == nullptr)) return CPLXAMD_EINVAL;
  const int Hs = H + 2 * pad_h - dil_h * (KH - 1), Ws = W + 2 * pad_w - dil_w * (KW - 1);   // the smaller image
  if (KW != 3 || C % 16 || N % 64 || (KH * (C / 16)) % 6 || Hs <= 0 || Ws <= 0 || Hs > H || Ws > W ||
      (KW - 1) * dil_w > 64 || KH > 8)
    return CPLXAMD_ESHAPE;
  const int64_t P = B * H * W;
  if (P == 0) return 0;
  const int64_t halo = ((int64_t)dil_h * (KH - 1) * W + dil_w * (KW - 1) + TM) * C * 2;
  if (P >= ((int64_t)1 << 31) - TM || P * C * 2 + 2 * halo >= (int64_t)0xF0000000) return CPLXAMD_ESHAPE;
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (!a16(w_packed) || !a16(ws)) return CPLXAMD_EALIGN;
  for (int pl = 0; pl < NP; ++pl)
    if (!a16(x[pl]) || !a16(y[pl]) || !a16(bias[pl])) return CPLXAMD_EALIGN;
  if (!ws || ws_bytes < cl_ws_bytes<CPLX>(N)) return CPLXAMD_EINVAL;
  cl::Args<CPLX> g{};
  for (int pl = 0; pl < NP; ++pl) { g.x[pl] = x[pl]; g.bias[pl] = bias[pl]; g.y[pl] = y[pl]; }
  g.w = w_packed; g.dump = ws;
  g.P = P;
  g.Hi = mode ? Hs : H; g.Wi = mode ? Ws : W; g.Ho = mode ? H : Hs; g.Wo = mode ? W : Ws;
  g.x_bytes = (uint32_t)(B * g.Hi * g.Wi * C * 2);
  if (mode) { pad_h = dil_h * (KH - 1) - pad_h; pad_w = dil_w * (KW - 1) - pad_w; }
  g.w_bytes = (uint32_t)cl_pack_bytes<CPLX>(N, C, KH, KW);
  g.H = H; g.W = W; g.C = C; g.Cout = N; g.KH = KH; g.dil_h = dil_h; g.dil_w = dil_w; g.pad_h = pad_h; g.pad_w = pad_w;
  g.C16 = C / 16; g.NS = KH * g.C16;
  g.tm_out = TM - (KW - 1) * dil_w;
  g.tiles_m = (int)((P + g.tm_out - 1) / g.tm_out);
  g.tiles_n = N / 64;
  g.div_w = make_div((uint32_t)W); g.div_h = make_div((uint32_t)H);
  const int ncu = device_cus() & ~7;
  const int64_t ntiles = (int64_t)g.tiles_m * g.tiles_n;
  if (ntiles > 0x7fffffff) return CPLXAMD_ESHAPE;
  // chip shared with RCCL collectives (CPLXAMD_LAUNCH_SHARED, launch.h): one workgroup per tile
  int grid = (ntiles < ncu || !launch_owns_chip(flags)) ? (int)ntiles : ncu;
  // Start stagger.  A tile takes ~ NS stages x 2 waves per SIMD x (3 taps x GRP x MPG) MFMAs x 32 clocks / 0.5; the
  // workgroups that get one tile less than the longest ones (ntiles % grid != 0) have that much slack: their starts are
  // spread over it.
  g.stagger = 0; g.stagger_from = 0;
  if (ntiles > 2 * grid && ntiles % grid) {
    const int64_t tile_clk = (int64_t)g.NS * 2 * (3 * G3::GRP * G3::MPG) * 32 * 2;
    g.stagger_from = (int)(ntiles % grid);
    g.stagger = (int)(tile_clk / (grid - g.stagger_from));
  }
  static PerDeviceOnce attr_set;
  if (const int e = set_max_dyn_lds(attr_set, cl::conv_cl_kernel<3, CPLX>, G3::SMEM)) return e;
  cl::conv_cl_kernel<3, CPLX><<<dim3((unsigned)grid), cl::NT, G3::SMEM, (hipStream_t)stream>>>(g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int cplxamd_cl_to_nchw(const void* x_cl, void* out, int64_t B, int C, int64_t S, void* stream) {
  if (!x_cl || !out || B < 0 || C <= 0 || S <= 0) return CPLXAMD_EINVAL;
  if (C % 8 || S % 8 || B * ((C + 63) / 64) > 65535) return CPLXAMD_ESHAPE;
  if ((reinterpret_cast<uintptr_t>(x_cl) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return CPLXAMD_EALIGN;
  if (B == 0) return 0;
  dim3 grid((unsigned)((S + 63) / 64), (unsigned)(B * ((C + 63) / 64)));
  cl::cl_to_nchw_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)x_cl, (bf16_t*)out, C, S);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

int64_t cplxamd_conv2d_cl_pack_bytes(int N, int C, int KH, int KW) { return cl_pack_bytes<true>(N, C, KH, KW); }
int64_t cplxamd_conv2d_clr_pack_bytes(int N, int C, int KH, int KW) { return cl_pack_bytes<false>(N, C, KH, KW); }
int64_t cplxamd_conv2d_cl_ws_bytes(int Cout) { return cl_ws_bytes<true>(Cout); }
int64_t cplxamd_conv2d_clr_ws_bytes(int Cout) { return cl_ws_bytes<false>(Cout); }

int cplxamd_conv2d_cl_pack(const void* w_r, const void* w_i, void* out, int Co, int Ci, int KH, int KW, int dgrad,
                           void* stream) {
  return cl_pack<true>(w_r, w_i, out, Co, Ci, KH, KW, dgrad, stream);
}
int cplxamd_conv2d_clr_pack(const void* w, void* out, int Co, int Ci, int KH, int KW, int dgrad, void* stream) {
  return cl_pack<false>(w, nullptr, out, Co, Ci, KH, KW, dgrad, stream);
}

// Forward (mode 0):  y[b, ho, wo, n] = bias[n] + sum_{kh, kw, c} x[b, ho + kh dil_h - pad_h, wo + kw dil_w - pad_w, c] w[n, c, kh, kw]
// over the taps inside the H x W image; x: [B][H][W][C], y: [B][Ho][Wo][N] with Ho = H + 2 pad_h - dil_h (KH - 1) <= H
// (likewise Wo): any zero padding up to `same`.  Data gradient (mode 1) OF THAT convolution: x is the output gradient
// [B][Ho][Wo][C = Cout], y the input gradient [B][H][W][N = Cin], w packed with dgrad = 1; H, W, pad_* are still the
// forward's.  ESHAPE for what the kernel is not built for (the caller falls back to conv_nhwc / conv_bf16).
int cplxamd_conv2d_cl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                      void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                      int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, void* stream) {
  return cplxamd_conv2d_cl_fl(x_r, x_i, w_packed, bias_r, bias_i, y_r, y_i, B, H, W, C, N, KH, KW, dil_h, dil_w, pad_h, pad_w,
                              mode, ws, ws_bytes, CPLXAMD_LAUNCH_DEFAULT, stream);
}

int cplxamd_conv2d_cl_fl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                         void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                         int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, int flags, void* stream) {
  return cl_launch<true>({x_r, x_i}, w_packed, {bias_r, bias_i}, {y_r, y_i}, B, H, W, C, N, KH, KW, dil_h, dil_w, pad_h, pad_w,
                         mode, ws, ws_bytes, flags, stream);
}

// The real-valued cplxamd_conv2d_cl: same arguments (one plane each), same conditions.
int cplxamd_conv2d_clr(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int H, int W, int C,
                       int N, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, int mode, void* ws,
                       int64_t ws_bytes, void* stream) {
  return cplxamd_conv2d_clr_fl(x, w_packed, bias, y, B, H, W, C, N, KH, KW, dil_h, dil_w, pad_h, pad_w, mode, ws, ws_bytes,
                               CPLXAMD_LAUNCH_DEFAULT, stream);
}

int cplxamd_conv2d_clr_fl(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int H, int W, int C,
                          int N, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, int mode, void* ws,
                          int64_t ws_bytes, int flags, void* stream) {
  return cl_launch<false>({x, nullptr}, w_packed, {bias, nullptr}, {y, nullptr}, B, H, W, C, N, KH, KW, dil_h, dil_w, pad_h,
                          pad_w, mode, ws, ws_bytes, flags, stream);
}

}  // extern "C"
