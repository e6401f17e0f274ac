// fp32-faithful implicit-GEMM convolution on the bf16 matrix pipe ("3xbf16 split, 6 products").
//
// gfx950 has no TF32/xf32 path and its fp32 MFMA runs at 1/16 of the bf16 rate (157 TFLOP/s peak).  Every fp32
// operand x is therefore pre-split into three bf16 planes  x = x1 + x2 + x3  (each the round-to-nearest bf16 of the
// running residual, |x - x1 - x2 - x3| <= 2^-27 |x|; the residuals are exact in fp32), and
//     a*b = a1b1 + (a1b2 + a2b1) + (a1b3 + a2b2 + a3b1)  + O(2^-26 |ab|)
// is evaluated with six v_mfma_f32_32x32x16_bf16 per fragment pair.  bf16 x bf16 products are exact in fp32; the
// six products are issued smallest-first into one accumulator that is folded into a total every 256 k (two-level
// accumulation as in the fp32 kernel).  Six bf16 MFMAs cost 192 cycles per 16 k against 512 for v_mfma_f32_32x32x2_f32: 2.67x the fp32 matrix rate at
// fp32-level accuracy (checked against fp64 in tests/test_ops_gpu.py with the same 2e-6 bar as the fp32 kernel).
//
// The split is a separate HBM-bound pass (sp_split3_bf16: 4 B read + 6 B written per element), amortised because each
// activation / gradient / weight tensor feeds GEMMs with thousands of FLOPs per element; planes are ordinary NHWC /
// [N][K] bf16 tensors.  With six MFMAs per fragment pair the kernel is MFMA-paced by construction (0.5 ds_read_b128 per
// MFMA); what limits it is operand delivery (per-CU L2/Infinity-Cache rate and the LDS store path), hence the tall
// 256x128x16 block tile, LDS-DMA staging and the source-side swizzle described at b3_kernel.
#include "common.h"
#include <algorithm>
#include <cstdlib>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

// Operand storage ("split-3 interleaved"): for every row (pixel / output channel) and every group of 16 consecutive k
// the three planes lie next to each other:  [row][k/16][plane 0..2][16 bf16]  = 96 contiguous bytes per (row, K-tile),
// so one K-tile of a block row is fetched as six consecutive 16-byte chunks (coalesced, L2-line friendly).
struct B3Args {
    const uint16_t* X;    // [pixels][Kc/16][3][16]
    const uint16_t* W;    // [Nout][K/16][3][16], row stride ldw3 elements (= 3*K)
    const float* bias;
    float* C;
    int64_t M;
    int Hi, Wi, Kc, ldx3;          // ldx3 = elements per pixel row of X (= 3*Kc)
    int Ho, Wo, Nout, ldc;
    int KH, KW, stride, pad, dil;
    int64_t ldw3;
    int ncblk, nkt, tiles_n;
    float alpha;
    int beta, relu;
    int dbg;              // timing experiments only (env SP_B3_DBG): 1 = no global loads, 2 = no MFMAs
    uint32_t x_bytes, w_bytes;   // data bytes of the split operands; a 64-byte zero block follows each (masked lanes)
};

// Block tile 256 x 128 x 16, 512 threads = 8 waves (4 along M x 2 along N, wave tile 64x64 = 2x2 MFMA tiles), 2 waves per
// SIMD, 1 workgroup per CU.  Why this shape and this staging:
//  * with six bf16 MFMAs per fragment pair a 128x128 tile needs ~64 GB/s of operand traffic per CU, more than
//    L2/Infinity Cache deliver per CU (v1 measured 30 GB/s = the Infinity-Cache rate, 32 % MFMA issue).  A 256-row tile halves
//    the weight traffic (the operand that streams from Infinity Cache) and keeps the activation panel in the XCD's L2 (the
//    N-tiles of one M-tile are adjacent in the XCD-remapped block order);
//  * register staging + ds_write_b128 (v2) spent ~700 LDS cycles per K-tile on the 79 B/clk VGPR->LDS store path next to
//    1536 MFMA cycles.  v3 stages with LDS-DMA (global_load_lds_dwordx4): no VGPRs, no ds_write, loads stay in flight
//    across the barrier behind a counted s_waitcnt vmcnt(N) in a 3-stage ring;
//  * LDS-DMA writes lane-linear (base + lane*16), so the LDS image is the linear [row][6 chunks] image of the operand and
//    bank conflicts are removed on the SOURCE side: chunk c of row r is stored at position (c + ((r>>3)&1)) mod 6 of its
//    row, which makes the 16 rows of every ds_read_b128 lane group ({0-3,12-15,20-27} / {4-11,16-19,28-31}) hit 16
//    distinct 16-byte slots of the 256-byte bank row (checked exhaustively in DESIGN.md) -- the same rotation is applied
//    to the fragment read address.
constexpr int BM = 256, BN = 128, BK = 16;
constexpr int A_BYTES = BM * 96;                 // 24576: [row][6 x 16 B]
constexpr int B_BYTES = BN * 96;                 // 12288
constexpr int STAGE_B = A_BYTES + B_BYTES;       // 36864
constexpr int NSTAGE = 4;                        // ring depth: NSTAGE-1 K-tiles in flight (147 KB LDS)
constexpr int CHUNK_KT = 16;                     // fold acc into tot every 16 K-tiles (256 k)

__device__ uint4 g_zero_page[4];                 // masked (zero-padding / out-of-range) lanes fetch from here

#define SP_GLDS16(src, dst)                                                                                      \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),                       \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

template <int MODE, int DBG>
__global__ __launch_bounds__(512, 2) void b3_kernel(B3Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    int tn, tmi;
    supertile_map(lid, gridDim.x / p.tiles_n, p.tiles_n, tmi, tn);
    const int64_t m0 = (int64_t)tmi * BM;
    const int n0 = tn * BN;
    // ---- loader mapping: LDS chunk g = t + 512 j  ->  row g/6, position g%6; source chunk = position un-rotated.
    // Address generation is kept off the per-K-tile path: a lane's byte offset (32 bit) and its validity depend only on
    // the filter tap and are recomputed when the tap changes (every Kc/16 K-tiles); per K-tile the wave adds a SCALAR
    // channel-block / k offset to the base, and masked lanes (zero padding, tile tails) are redirected to the 64-byte
    // zero block that follows the operand, so every lane uses the same scalar-base + 32-bit-offset addressing. ----
    const int HoWo = p.Ho * p.Wo;
    int a_c8[3], a_py[3], a_px[3], a_boff[3];
    bool a_rowok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int idx = t + 512 * j;
        const int row = idx / 6, pos = idx - row * 6;
        a_c8[j] = ((pos + 6 - ((row >> 3) & 1)) % 6) * 16;            // byte offset of the source chunk in its 96-B group
        const int64_t m = m0 + row;
        a_rowok[j] = m < p.M;
        const int64_t mm = a_rowok[j] ? m : 0;
        const int b = (int)(mm / HoWo);
        const int rem = (int)(mm - (int64_t)b * HoWo);
        const int yo = rem / p.Wo, xo = rem - yo * p.Wo;
        a_boff[j] = b * p.Hi * p.Wi;
        if (MODE == 0) {
            a_py[j] = yo * p.stride - p.pad;
            a_px[j] = xo * p.stride - p.pad;
        } else {
            a_py[j] = yo + p.pad;
            a_px[j] = xo + p.pad;
        }
    }
    uint32_t b_voff[2];
    bool b_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = t + 512 * j;
        const int row = idx / 6, pos = idx - row * 6;
        const int c8 = ((pos + 6 - ((row >> 3) & 1)) % 6) * 16;
        b_ok[j] = idx < BN * 6 && (n0 + row) < p.Nout;
        b_voff[j] = b_ok[j] ? (uint32_t)((int64_t)(n0 + row) * p.ldw3 * 2 + c8) : 0u;
    }
    int ld_ky = 0, ld_kx = 0, ld_cblk = 0, ld_kt = 0;
    uint32_t a_voff[3];
    bool a_ok[3];
    const int rowbytes = p.ldx3 * 2;

    auto tap_update = [&]() {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bool ok = a_rowok[j];
            int iy, ix;
            if (MODE == 0) {
                iy = a_py[j] + ld_ky * p.dil;
                ix = a_px[j] + ld_kx * p.dil;
                ok = ok && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
            } else {
                const int ty = a_py[j] - ld_ky * p.dil, tx = a_px[j] - ld_kx * p.dil;
                ok = ok && ty >= 0 && tx >= 0;
                if (p.stride == 1) {
                    iy = ty;
                    ix = tx;
                } else {
                    iy = ty / p.stride;
                    ix = tx / p.stride;
                    ok = ok && (iy * p.stride == ty) && (ix * p.stride == tx);
                }
                ok = ok && iy < p.Hi && ix < p.Wi;
            }
            a_ok[j] = ok;
            a_voff[j] = ok ? (uint32_t)(a_boff[j] + iy * p.Wi + ix) * (uint32_t)rowbytes + (uint32_t)a_c8[j] : 0u;
        }
    };

    auto issue_tile = [&](int stage) {
        unsigned char* st = smem + stage * STAGE_B;
        if (ld_cblk == 0) tap_update();
        const uint32_t koffA = (uint32_t)ld_cblk * 96u;                  // scalar: channel block inside the pixel row
        const unsigned char* baseA = reinterpret_cast<const unsigned char*>(p.X) + koffA;
        const uint32_t zrelA = p.x_bytes - koffA;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t off = a_ok[j] ? a_voff[j] : zrelA;
            if constexpr (DBG == 3) {
                const uint4 v = *reinterpret_cast<const uint4*>(baseA + off);
                asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            } else {
                SP_GLDS16(baseA + off, st + (wave + 8 * j) * 1024);
            }
        }
        const uint32_t koffB = (uint32_t)ld_kt * 96u;
        const unsigned char* baseB = reinterpret_cast<const unsigned char*>(p.W) + koffB;
        const uint32_t zrelB = p.w_bytes - koffB;
        {
            const uint32_t off = b_ok[0] ? b_voff[0] : zrelB;
            if constexpr (DBG == 3) {
                const uint4 v = *reinterpret_cast<const uint4*>(baseB + off);
                asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            } else {
                SP_GLDS16(baseB + off, st + A_BYTES + wave * 1024);
            }
        }
        if (wave < 4) {
            const uint32_t off = b_ok[1] ? b_voff[1] : zrelB;
            if constexpr (DBG == 3) {
                const uint4 v = *reinterpret_cast<const uint4*>(baseB + off);
                asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            } else {
                SP_GLDS16(baseB + off, st + A_BYTES + (wave + 8) * 1024);
            }
        }
        ++ld_kt;
        if (++ld_cblk == p.ncblk) {
            ld_cblk = 0;
            if (++ld_kx == p.KW) {
                ld_kx = 0;
                ++ld_ky;
            }
        }
    };

    // fragment read offsets: row r, chunk c = 2*plane + h stored at position (c + ((r>>3)&1)) % 6
    const int rot = (l32 >> 3) & 1;
    int offA[3], offB[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int pos = (2 * q + h + rot) % 6;
        offA[q] = (wm * 64 + l32) * 96 + pos * 16;
        offB[q] = A_BYTES + (wn * 64 + l32) * 96 + pos * 16;
    }

    f32x16 tot[2][2], acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tot[i][j][r] = 0.f;
                acc[i][j][r] = 0.f;
            }

    // prologue: tiles 0 and 1 in flight, tile 0 landed
    constexpr bool do_load = DBG != 1, do_mma = DBG != 2;
    int issued = 0;
    if (do_load)
        for (; issued < NSTAGE - 1 && issued < p.nkt; ++issued) issue_tile(issued);
    // wait until tile 0 has landed: all but the (issued-1) newest tiles
    if (issued >= 3) {
        if (wave < 4) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (issued == 2) {
        if (wave < 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    int stage = 0;
    for (int kt = 0; kt < p.nkt; ++kt) {
        // prefetch tile kt+NSTAGE-1 into the stage that was read in iteration kt-1 (all waves passed the barrier since)
        const bool pre = kt + NSTAGE - 1 < p.nkt;
        const unsigned char* st = smem + stage * STAGE_B;
        bf16x8 af[2][3], bf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                af[i][q] = *reinterpret_cast<const bf16x8*>(st + offA[q] + i * 32 * 96);
                bf[i][q] = *reinterpret_cast<const bf16x8*>(st + offB[q] + i * 32 * 96);
            }
        if constexpr (do_mma)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // six products, smallest magnitude first (a1b3, a3b1, a2b2 ~2^-18; a1b2, a2b1 ~2^-9; a1b1)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][2], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], bf[j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
            }
        // Prefetch of tile kt+NSTAGE-1 is issued BEHIND the MFMAs in program order: a load whose issue is back-pressured by the
        // memory queue then stalls the wave while the matrix pipe still has this wave's (and its SIMD partner's) MFMAs queued,
        // instead of in front of the fragment reads with the pipe idle (measured: fwd 8.06 -> 7.58 ms, wgrad 10.99 -> 8.40 ms).
        if (pre && do_load) issue_tile(stage == 0 ? NSTAGE - 1 : stage - 1);
        if constexpr (!do_mma) {   // keep the fragment reads alive in the no-MFMA timing mode
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 3; ++q) asm volatile("" ::"v"(af[i][q]), "v"(bf[i][q]));
        }
        if ((kt & (CHUNK_KT - 1)) == CHUNK_KT - 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        // tile kt+1 must have landed: everything but the NSTAGE-2 newest tiles (fewer near the end), then rendezvous
        {
            const int newer = min(NSTAGE - 2, p.nkt - 2 - kt);      // tiles younger than kt+1 that are in flight
            if (newer >= 2) {
                if (wave < 4) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            } else if (newer == 1) {
                if (wave < 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage = (stage == NSTAGE - 1) ? 0 : stage + 1;
    }

#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + l32;
        if (n >= p.Nout) continue;
        const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < p.M) {
                    float* dst = p.C + m * p.ldc + n;
                    float v = p.alpha * (tot[i][j][r] + acc[i][j][r]) + bv;
                    if (p.beta) v += *dst;
                    if (p.relu) v = fmaxf(v, 0.f);
                    *dst = v;
                }
            }
        }
    }
}

// ================================================================================================================
// Weight gradient on the same scheme:  dW[co][tap][ci] = sum_m dY[m][co] * X[pix(m,tap)][ci]   (K = pixels).
// Both operands are pixel-major in HBM, so a K-tile (16 pixels) is staged as [pixel][channel chunks] rows by LDS-DMA and
// the K-major MFMA fragments are produced by ds_read_b64_tr_b16 (hardware transpose read: a 16-lane group reads a
// 4-pixel x 16-channel block and each lane receives one channel's 4 consecutive pixels; verified lane map in
// tools/probes/tr_probe.hip).  A pixel row is 1536 B (A: 256 co) / 768 B (B: 128 ci), both = 0 mod 256, so the four
// pixel rows of a block would collide on the same banks; the loader therefore stores row r rotated by 4*(r&3) chunks
// (64 B), which spreads the 4 rows x 2 channel groups of every 32-lane half over all 64 banks -> conflict-free.
// Block tile 256 (co) x 128 (tap,ci) x 16 pixels, 8 waves, 3-stage ring, counted vmcnt -- as the forward kernel.
// The pixel reduction is split over blockIdx.y into partial slabs (summed in a fixed order by wgrad3_reduce_kernel).
struct W3Args {
    const uint16_t* X;     // split-3 [pixels_in][Ci/16][3][16]
    const uint16_t* dY;    // split-3 [pixels_out][Co/16][3][16]
    float* out;            // dW [Co][ldo] or slabs
    int64_t M;             // output pixels
    int Hi, Wi, Ci, Ho, Wo, Co;
    int KH, KW, stride, pad, dil;
    int Ntot, ldo, tiles_n, splits;
    int64_t rows_per_split, slab_stride;
    float alpha;
    int beta;
    uint32_t x_bytes, y_bytes;   // data bytes of the split operands (zero block follows)
};

constexpr int WA_BYTES = 16 * 1536;              // 24576
constexpr int WB_BYTES = 16 * 768;               // 12288
constexpr int WSTAGE_B = WA_BYTES + WB_BYTES;    // 36864

typedef short short4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* base, int off0, int off1) {
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(base + off0));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(base + off1));
    typedef short short8v __attribute__((ext_vector_type(8)));
    short8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ __launch_bounds__(512, 2) void w3_kernel(W3Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = lid % p.tiles_n, tmi = lid / p.tiles_n;
    const int co0 = tmi * 256, n0 = tn * 128;
    const int tap = n0 / p.Ci, ci0 = n0 - tap * p.Ci;           // Ci % 128 == 0: a column tile lies inside one tap
    const int ky = tap / p.KW, kx = tap - ky * p.KW;
    const int split = blockIdx.y;
    const int64_t m_begin = (int64_t)split * p.rows_per_split;
    const int64_t m_end = min(p.M, m_begin + p.rows_per_split);
    const int nkt = (int)((m_end - m_begin + 15) / 16);
    const int HoWo = p.Ho * p.Wo;

    // ---- loader mapping (cheap per-K-tile addressing as in b3_kernel: 32-bit lane offsets + scalar base; masked lanes
    //      read the zero block after the operand; the pixel coordinates of the gathered operand advance incrementally) ----
    uint32_t a_voff[3];
    int a_r[3];
    bool a_cok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int g = t + 512 * j;
        const int r = g / 96, pos = g - r * 96;
        const int js = (pos + 96 - 4 * (r & 3)) % 96;            // un-rotate: which source chunk lands here
        a_r[j] = r;
        a_cok[j] = co0 + (js / 6) * 16 < p.Co;
        a_voff[j] = (uint32_t)r * (uint32_t)(6 * p.Co) + (uint32_t)(co0 * 6 + js * 16);    // bytes relative to pixel mt
    }
    int b_r[2], b_c8[2], b_b[2], b_y[2], b_x[2];
    bool b_live[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int g = t + 512 * j;
        const int r = (g / 48) & 15, pos = g % 48;
        const int js = (pos + 48 - 4 * (r & 3)) % 48;
        b_r[j] = r;
        b_c8[j] = ci0 * 6 + js * 16;
        b_live[j] = g < 768 && n0 + (js / 6) * 16 < p.Ntot;
        const int64_t m = m_begin + r;                            // coordinates of this lane's pixel in K-tile 0
        const int b = (int)(m / HoWo);
        const int rem = (int)(m - (int64_t)b * HoWo);
        b_b[j] = b;
        b_y[j] = rem / p.Wo;
        b_x[j] = rem - b_y[j] * p.Wo;
    }
    const int y_adv = 16 / p.Wo, x_adv = 16 - y_adv * p.Wo;      // advancing 16 output pixels = y_adv rows + x_adv columns
    const bool tiny_map = HoWo < 16;                              // a K-tile of 16 pixels can then cross several images
    const uint32_t xrow = (uint32_t)(6 * p.Ci);
    int ld_kt = 0;
    auto issue_tile = [&](int stage) {
        unsigned char* st = smem + stage * WSTAGE_B;
        const int64_t mt = m_begin + (int64_t)ld_kt * 16;
        const unsigned char* baseA = reinterpret_cast<const unsigned char*>(p.dY) + mt * (6 * (int64_t)p.Co);   // scalar
        const int64_t rem_bytes = (int64_t)p.y_bytes - mt * (6 * (int64_t)p.Co);
        const uint32_t zrelA = (uint32_t)rem_bytes;
        const int rows_left = (int)min((int64_t)16, m_end - mt);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool ok = a_cok[j] && a_r[j] < rows_left;
            SP_GLDS16(baseA + (ok ? a_voff[j] : zrelA), st + (wave + 8 * j) * 1024);
        }
        const unsigned char* baseB = reinterpret_cast<const unsigned char*>(p.X);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && wave >= 4) break;
            const int iy = b_y[j] * p.stride - p.pad + ky * p.dil, ix = b_x[j] * p.stride - p.pad + kx * p.dil;
            const bool ok = b_live[j] && b_r[j] < rows_left && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
            const uint32_t off = (uint32_t)((b_b[j] * p.Hi + iy) * p.Wi + ix) * xrow + (uint32_t)b_c8[j];
            SP_GLDS16(baseB + (ok ? off : p.x_bytes), st + WA_BYTES + (wave + 8 * j) * 1024);
            // advance this lane's pixel by 16 for the next K-tile (no divisions)
            b_x[j] += x_adv;
            b_y[j] += y_adv;
            if (b_x[j] >= p.Wo) { b_x[j] -= p.Wo; ++b_y[j]; }
            if (b_y[j] >= p.Ho) { b_y[j] -= p.Ho; ++b_b[j]; }      // maps of >= 16 pixels cross at most one image boundary per K-tile
            if (tiny_map)                                            // scalar condition: pure-GEMM uses of the kernel (Ho*Wo < 16)
                while (b_y[j] >= p.Ho) { b_y[j] -= p.Ho; ++b_b[j]; }
        }
        ++ld_kt;
    };

    // ---- transposed-read offsets: lane (group g4 = lane>>4, q = (lane>>2)&3, pp = lane&3) addresses pixel row
    //      8h + 4s + q, channels cbase + 16*(g4&1) + 4pp .. +3 of plane pl ------------------------------------------------
    const int g4 = (lane >> 4) & 1, q = (lane >> 2) & 3, pp = lane & 3;
    int offA[2][3][2], offB[2][3][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int row = 8 * h + 4 * s2 + q;
                const int ja = (wm * 4 + i * 2 + g4) * 6 + pl * 2 + (pp >> 1);
                offA[i][pl][s2] = row * 1536 + ((ja + 4 * q) % 96) * 16 + (pp & 1) * 8;
                const int jb = (wn * 4 + i * 2 + g4) * 6 + pl * 2 + (pp >> 1);
                offB[i][pl][s2] = WA_BYTES + row * 768 + ((jb + 4 * q) % 48) * 16 + (pp & 1) * 8;
            }

    f32x16 tot[2][2], acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tot[i][j][r] = 0.f;
                acc[i][j][r] = 0.f;
            }

    {
        int issued = 0;
        for (; issued < NSTAGE - 1 && issued < nkt; ++issued) issue_tile(issued);
        if (issued >= 3) {
            if (wave < 4) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else if (issued == 2) {
            if (wave < 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __builtin_amdgcn_s_barrier();

    int stage = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool pre = kt + NSTAGE - 1 < nkt;
        const unsigned char* st = smem + stage * WSTAGE_B;
        bf16x8 af[2][3], bf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                af[i][pl] = tr_pair(st, offA[i][pl][0], offA[i][pl][1]);
                bf[i][pl] = tr_pair(st, offB[i][pl][0], offB[i][pl][1]);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][2], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], bf[j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], bf[j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
            }
        if (pre) issue_tile(stage == 0 ? NSTAGE - 1 : stage - 1);     // behind the MFMAs (see b3_kernel)
        if ((kt & (CHUNK_KT - 1)) == CHUNK_KT - 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        {
            const int newer = min(NSTAGE - 2, nkt - 2 - kt);      // tiles younger than kt+1 that are in flight
            if (newer >= 2) {
                if (wave < 4) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            } else if (newer == 1) {
                if (wave < 4) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage = (stage == NSTAGE - 1) ? 0 : stage + 1;
    }

    float* out = p.out + (p.splits > 1 ? (int64_t)split * p.slab_stride : 0);
    const bool direct = p.splits == 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + l32;
        if (n >= p.Ntot) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < p.Co) {
                    float* dst = out + (int64_t)co * p.ldo + n;
                    const float v = tot[i][j][r] + acc[i][j][r];
                    if (direct) {
                        float w = p.alpha * v;
                        if (p.beta) w += *dst;
                        *dst = w;
                    } else {
                        *dst = v;
                    }
                }
            }
        }
    }
}

__global__ void wgrad3_reduce_kernel(const float* slab, float* out, int Co, int Ntot, int ldo, int splits, int64_t slab_stride,
                                     float alpha, int beta) {
    const int64_t total = (int64_t)Co * Ntot;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i / Ntot), n = (int)(i - (int64_t)co * Ntot);
        const int64_t off = (int64_t)co * ldo + n;
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += slab[(int64_t)k * slab_stride + off];
        s *= alpha;
        if (beta) s += out[off];
        out[off] = s;
    }
}

int w3_splits(const sp_wgrad_desc* d) {
    const int64_t M = (int64_t)d->N_img * d->Ho * d->Wo;
    const int64_t tiles = sp_cdiv(d->Co, 256) * sp_cdiv((int64_t)d->KH * d->KW * d->Ci, 128);
    int64_t want = sp_cdiv(2048, tiles);                          // 1 workgroup per CU: aim for >= 8 rounds of 256
    want = std::min<int64_t>(want, std::max<int64_t>(1, M / 512));  // >= 32 K-tiles per split
    want = std::min<int64_t>(want, 64);
    return (int)std::max<int64_t>(1, want);
}

// ---- split kernels ------------------------------------------------------------------------------------------
__device__ __forceinline__ void split3(float v, uint16_t& a, uint16_t& b, uint16_t& c) {
    const __bf16 x1 = (__bf16)v;
    const float r1 = v - (float)x1;
    const __bf16 x2 = (__bf16)r1;
    const float r2 = r1 - (float)x2;
    const __bf16 x3 = (__bf16)r2;
    a = __builtin_bit_cast(uint16_t, x1);
    b = __builtin_bit_cast(uint16_t, x2);
    c = __builtin_bit_cast(uint16_t, x3);
}

// x fp32 [rows][K] (K % 16 == 0)  ->  [rows][K/16][3][16] bf16.  One thread per 4 consecutive k.
__global__ __launch_bounds__(256) void split3_kernel(const float* x, int64_t n4, uint16_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        ushort4 a, b, c;
        split3(v.x, a.x, b.x, c.x);
        split3(v.y, a.y, b.y, c.y);
        split3(v.z, a.z, b.z, c.z);
        split3(v.w, a.w, b.w, c.w);
        const int64_t g = i >> 2;            // 16-k group (global, rows are multiples of 16 long)
        const int sub = (int)(i & 3) * 4;    // offset inside the group
        uint16_t* o = out + g * 48 + sub;
        *reinterpret_cast<ushort4*>(o) = a;
        *reinterpret_cast<ushort4*>(o + 16) = b;
        *reinterpret_cast<ushort4*>(o + 32) = c;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8)       // 64-byte zero block right after the data (masked lanes of the GEMM loaders)
        reinterpret_cast<uint2*>(out + 12 * n4)[threadIdx.x] = make_uint2(0u, 0u);
}

// w [Co][taps][Ci] fp32 -> rows n = ci, k = (tap, co):  [Ci][taps*Co/16][3][16]  (the K-contiguous B operand of dgrad)
__global__ __launch_bounds__(256) void split3_wT_kernel(const float* w, int Co, int taps, int Ci, uint16_t* out) {
    const int64_t total = (int64_t)Co * taps * Ci;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Co);
        int64_t r = i / Co;
        const int tap = (int)(r % taps);
        const int ci = (int)(r / taps);
        uint16_t a, b, c;
        split3(w[((int64_t)co * taps + tap) * Ci + ci], a, b, c);
        const int64_t k = (int64_t)tap * Co + co;                      // k index inside row ci
        uint16_t* o = out + ((int64_t)ci * ((int64_t)taps * Co / 16) + (k >> 4)) * 48 + (k & 15);
        o[0] = a;
        o[16] = b;
        o[32] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) reinterpret_cast<uint2*>(out + 3 * total)[threadIdx.x] = make_uint2(0u, 0u);
}

template <int MODE, int DBG>
int launch_b3(const B3Args& a, hipStream_t s) {
    constexpr int lds = NSTAGE * STAGE_B;
    return sp_launch_lds<b3_kernel<MODE, DBG>, lds>({sp_cdiv(a.M, BM) * a.tiles_n}, 512, lds, s, a);
}

}  // namespace

extern "C" int sp_split3_bf16(const float* x, int64_t n, void* out, void* stream) {
    if (!x || !out) return SP_ENULL;
    if (n % 16) return SP_EINVAL;            // every row must be a multiple of 16 long
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(split3_kernel, dim3(sp_ew_grid(n4, 4096)), dim3(256), 0, (hipStream_t)stream, x, n4, (uint16_t*)out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_split3_bf16_wT(const float* w, int Co, int taps, int Ci, void* out, void* stream) {
    if (!w || !out) return SP_ENULL;
    if (((int64_t)taps * Co) % 16) return SP_EINVAL;
    const int64_t total = (int64_t)Co * taps * Ci;
    hipLaunchKernelGGL(split3_wT_kernel, dim3(sp_ew_grid(total, 4096)), dim3(256), 0, (hipStream_t)stream, w, Co, taps, Ci, (uint16_t*)out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_conv_igemm_bf16x3(const sp_conv_desc* d, const void* Xs, const void* Ws, const float* bias, float* out,
                                    void* stream) {
    if (!d || !Xs || !Ws || !out) return SP_ENULL;
    if (d->mode != 0 && d->mode != 1) return SP_EINVAL;
    if (d->Kc % 16 || d->ldx != d->Kc) return SP_EINVAL;
    if (((uintptr_t)Xs | (uintptr_t)Ws) & 15) return SP_EINVAL;
    if (d->nbatch != 1 || d->stride < 1 || d->dil < 1) return SP_EINVAL;
    B3Args a;
    a.X = (const uint16_t*)Xs; a.W = (const uint16_t*)Ws; a.bias = bias; a.C = out;
    a.M = (int64_t)d->N_img * d->Ho * d->Wo;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Kc = d->Kc; a.ldx3 = 3 * d->Kc;
    a.Ho = d->Ho; a.Wo = d->Wo; a.Nout = d->Nout; a.ldc = d->ldc;
    a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
    a.ldw3 = 3 * (int64_t)d->KH * d->KW * d->Kc;
    a.ncblk = d->Kc / 16;
    a.nkt = d->KH * d->KW * a.ncblk;
    a.tiles_n = (int)sp_cdiv(d->Nout, BN);
    a.alpha = d->alpha; a.beta = d->beta; a.relu = d->relu;
    const int64_t xb = 6LL * d->N_img * d->Hi * d->Wi * d->Kc, wb = 6LL * d->Nout * d->KH * d->KW * d->Kc;
    if (!sp_span32_ok(xb, wb)) return SP_EINVAL;
    a.x_bytes = (uint32_t)xb; a.w_bytes = (uint32_t)wb;
    a.dbg = 0;
    if (a.M <= 0 || a.Nout <= 0) return SP_EINVAL;
#ifdef SP_TIMING_VARIANTS      // wrong-result timing modes: timing build only (sp_set_tuning("b3_dbg", n))
    const int dbg = sp_tuning_get(SP_TUNE_B3_DBG, 0);
    a.dbg = dbg;
    if (dbg == 1) return d->mode == 0 ? launch_b3<0, 1>(a, (hipStream_t)stream) : launch_b3<1, 1>(a, (hipStream_t)stream);
    if (dbg == 2) return d->mode == 0 ? launch_b3<0, 2>(a, (hipStream_t)stream) : launch_b3<1, 2>(a, (hipStream_t)stream);
    if (dbg == 3) return d->mode == 0 ? launch_b3<0, 3>(a, (hipStream_t)stream) : launch_b3<1, 3>(a, (hipStream_t)stream);
#endif
    return d->mode == 0 ? launch_b3<0, 0>(a, (hipStream_t)stream) : launch_b3<1, 0>(a, (hipStream_t)stream);
}

extern "C" int64_t sp_conv_wgrad_bf16x3_workspace(const sp_wgrad_desc* d) {
    if (!d) return 0;
    const int sp = w3_splits(d);
    return sp <= 1 ? 0 : (int64_t)sp * d->Co * d->ldo * (int64_t)sizeof(float);
}

extern "C" int sp_conv_wgrad_bf16x3(const sp_wgrad_desc* d, const void* Xsplit, const void* dYsplit, float* dW, void* workspace,
                                    void* stream) {
    if (!d || !Xsplit || !dYsplit || !dW) return SP_ENULL;
    if (d->Ci % 128 || d->Co % 16 || d->ldx != d->Ci || d->ldy != d->Co || d->nbatch != 1) return SP_EINVAL;
    if (((uintptr_t)Xsplit | (uintptr_t)dYsplit) & 15) return SP_EINVAL;
    W3Args a;
    a.X = (const uint16_t*)Xsplit; a.dY = (const uint16_t*)dYsplit;
    sp_fill_wgrad_geom(a, d, (int64_t)d->N_img * d->Ho * d->Wo, w3_splits(d), 16);
    a.stride = d->stride;
    a.tiles_n = (int)sp_cdiv(a.Ntot, 128);
    if (a.splits > 1 && !workspace) return SP_ENULL;
    a.out = a.splits > 1 ? (float*)workspace : dW;
    a.alpha = d->alpha; a.beta = d->beta;
    if (a.M <= 0) return SP_EINVAL;
    const int64_t xb = 6LL * d->N_img * d->Hi * d->Wi * d->Ci, yb = 6LL * a.M * d->Co;
    if (!sp_span32_ok(xb, yb) || d->Ho * d->Wo < 1) return SP_EINVAL;
    a.x_bytes = (uint32_t)xb; a.y_bytes = (uint32_t)yb;
    hipStream_t s = (hipStream_t)stream;
    constexpr int lds = NSTAGE * WSTAGE_B;
    const int rc = sp_launch_lds<w3_kernel, lds>({sp_cdiv(d->Co, 256) * a.tiles_n, a.splits}, 512, lds, s, a);
    if (rc != SP_OK) return rc;
    if (a.splits > 1) {
        const int64_t total = (int64_t)d->Co * a.Ntot;
        hipLaunchKernelGGL(wgrad3_reduce_kernel, dim3(sp_ew_grid(total, 4096)), dim3(256), 0, s, (const float*)workspace, dW, d->Co, a.Ntot,
                           d->ldo, a.splits, a.slab_stride, d->alpha, d->beta);
        SP_LAUNCH_CHECK();
    }
    return SP_OK;
}
