// What the four X C kernels share, written ONCE.
//
// k_contract_xc, k_contract_xc_row, k_contract_xc_256 (contract.hip) and k_contract_xc_lds (xclds.hip) differ in how they keep
// tiles of X in flight, and each keeps that to itself: its `issue` lambdas, the number and order of its global loads between
// waits, its sched_barriers, its ring and where its C fragments live.  The parts below take values that are already loaded and
// return values to store or accumulate; NONE of them loads X.  The only global memory they touch is the rows of B
// (b_rows_clamped: called where the kernel issued those loads itself, the same 4 NB loads), the fragment image of C at the
// index the kernel asks for, the two segment tables and the outputs XC, seg_rhs, seg_btb.  Every function is forced inline.
// Reference: decomposition.py:147-158 (X_i C, diag(B_i^T X_i C), B_i^T B_i) and :242.
#pragma once
#include <type_traits>

#include "mcl_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

static __device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// Wave-private LDS tile of 16 rows x W floats; the 16-byte slot index is XORed with the row, so the row-wise writes and the
// column-wise fragment reads are both conflict-free.
template <int W>
struct XcTile {
    // row `row`, logical 16-byte slot `slot`
    static __device__ __forceinline__ void put(float *L, int row, int slot, f32x4 v) {
        *reinterpret_cast<f32x4 *>(L + row * W + ((slot ^ row) << 2)) = v;
    }
    // MFMA A fragments of lane (q, i16): X[row i16][64 kc + 16 kq + 4 q .. + 3] of the tile
    static __device__ __forceinline__ f32x4 frag(const float *L, int i16, int q, int kc, int kq) {
        return *reinterpret_cast<const f32x4 *>(L + i16 * W + (((16 * kc + 4 * kq + q) ^ i16) << 2));
    }
};

// The fragment image of C (k_build_cfrag): the four floats m of 64-column chunk `chunk`, quarter kq, column block nb, lane
//   = C[64 chunk + 16 kq + 4 (lane >> 4) + m][16 nb + (lane & 15)], zero outside C
static __host__ __device__ __forceinline__ long cfrag_index(int chunk, int kq, int NB, int nb, int lane) {
    return ((((long)chunk * 4 + kq) * NB + nb) * 64 + lane) * 4;
}
// ... read from the image at `Cfrag`, in global memory or in LDS
template <int NB>
static __device__ __forceinline__ f32x4 cfrag_at(const float *Cfrag, int chunk, int kq, int nb, int lane) {
    return *reinterpret_cast<const f32x4 *>(Cfrag + cfrag_index(chunk, kq, NB, nb, lane));
}

// End of a 16-row block: the NCH independent fp32 chains of every output (one per 64-column chunk modulo 4) summed pairwise,
// and cleared for the next block.  Rank > 32 (NB == 4) has registers for one chain only.
template <int NCH, int NB>
static __device__ __forceinline__ void chains_sum4(f32x4 (&acc4)[NCH][NB], f32x4 (&acc)[NB]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        if (NCH == 4) acc[nb] = (acc4[0][nb] + acc4[1][nb]) + (acc4[2 % NCH][nb] + acc4[3 % NCH][nb]);
        else acc[nb] = acc4[0][nb];
#pragma unroll
        for (int kc = 0; kc < NCH; ++kc) acc4[kc][nb] = zero4();
    }
}

// Rows 16 blk + 4 q + v, columns bcolc[nb] of B for the block (row0, nrows, blk): 4 NB unconditional loads at rows clamped into
// the segment (bcolc is clamped by the caller); SegGram::block masks them at use
template <int NB>
static __device__ __forceinline__ void b_rows_clamped(const float *B, long row0, int blk, int nrows, int r, const int (&bcolc)[NB], int q,
                                                      float (&out)[NB][4]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long j = row0 + min(16 * blk + 4 * q + v, nrows - 1);
            out[nb][v] = B[j * r + bcolc[nb]];
        }
}

// The A-phase reductions fused into the X C pass, per SEGMENT (<= 256 rows of one slab; k_A_finish sums the segments of its
// slab): while a 16-row block of XC is still in the accumulators (lane (q, i16) holds rows 4q + v, column 16 nb + i16),
//     rhs_seg[c] += sum_rows B[row][c] XC[row][c]      (diag(B_i^T X_i C))
//     BtB_seg    += B_blk^T B_blk                      (A = B-operand = b[v], reduction index <-> the 4 lane quarters)
// GRAM == 2 (penalty-free A: its systems are not shifted and amplify every relative error of these sums): fp64 throughout - the
// products b * xc and b * b' of fp32 values are exact in fp64, so the only rounding left in rhs_i and B_i^T B_i is the fp32
// rounding of X C itself.  GRAM == 1 (penalised A): fp32 chains over the segment's <= 256 rows (4 fp32 MFMAs per block instead
// of 4 NB^2 fp64 ones at twice the cycles: 12 % of the kernel at rank 32), widened to fp64 when the segment is stored.
// GRAM == 0: the XC store alone.
// k_contract_xc_256 and k_contract_xc_lds use this struct.  k_contract_xc_row holds the same text (with that of chains_sum4) in its
// own body - called from there, it changed the waits of that kernel's unfenced forms - so a change here is made there too.
template <int NB, int GRAM>
struct SegGram {
    double p[NB];
    float pf[NB];
    f64x4 accG[NB][NB];
    f32x4 accGf[NB][NB];

    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int a = 0; a < NB; ++a) {
            p[a] = 0.0, pf[a] = 0.f;
#pragma unroll
            for (int b = 0; b < NB; ++b) accG[a][b] = f64x4{0.0, 0.0, 0.0, 0.0}, accGf[a][b] = zero4();
        }
    }

    // block `blk` of segment (row0, nrows): stores acc as XC and accumulates the reductions with bcur, the block's rows of B as
    // b_rows_clamped loaded them.  ONE mask guards the store and zeroes b: rows past the segment, columns past the rank.
    __device__ __forceinline__ void block(const f32x4 (&acc)[NB], const float (&bcur)[NB][4], long row0, int blk, int nrows, int r,
                                          float *XC, int q, int i16) {
        float bv[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = 16 * nb + i16;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rl = 16 * blk + 4 * q + v;
                const long j = row0 + rl;
                const bool ok = (rl < nrows) && (col < r);
                if (ok) XC[j * r + col] = acc[nb][v];
                if (GRAM) {
                    const float b = ok ? bcur[nb][v] : 0.f;
                    bv[nb][v] = b;
                    if (GRAM == 2) p[nb] = fma((double)b, (double)acc[nb][v], p[nb]);
                    else pf[nb] = fmaf(b, acc[nb][v], pf[nb]);
                }
            }
        }
        if (GRAM) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int a = 0; a < NB; ++a)
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        if (GRAM == 2)
                            accG[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)bv[a][v], (double)bv[b][v], accG[a][b], 0, 0, 0);
                        else
                            accGf[a][b] = MFMA16(bv[a][v], bv[b][v], accGf[a][b]);
                    }
        }
    }

    // the sums of segment sg go out (the caller resets)
    __device__ __forceinline__ void store(int sg, int r, double *seg_rhs, double *seg_btb, int q, int i16) const {
        if (!GRAM) return;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            double t = (GRAM == 2) ? p[nb] : (double)pf[nb];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            const int col = 16 * nb + i16;
            if (q == 0 && col < r) seg_rhs[(long)sg * r + col] = t;
        }
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    // D layouts: f64 MFMA row = (l >> 4) + 4 reg, f32 MFMA row = 4 (l >> 4) + reg; col = l & 15
                    const int ra = 16 * a + ((GRAM == 2) ? q + 4 * v : 4 * q + v), cb = 16 * b + i16;
                    const double val = (GRAM == 2) ? accG[a][b][v] : (double)accGf[a][b][v];
                    if (ra < r && cb < r) seg_btb[((long)sg * r + ra) * r + cb] = val;
                }
    }
};

// A wave's position in the flat walk over its segments [s0, s1): segment, 16-row block, tile `hs` of `tpb` in the block
// (k_contract_xc_256: tpb = 1).  Wave-uniform.  Past the wave's last tile the cursor parks at blk = nblk: loads issued from it
// clamp to the last row of the last segment, and nothing is stored from it.
struct SegCursor {
    const int *seg_row0, *seg_rows;
    int sg, s1, nrows, nblk, blk, hs;
    long row0;

    // the wave's segments [s0, s1_) of the two tables; the cursor stands on the first tile of s0
    __device__ __forceinline__ void begin(const int *row0_tab, const int *rows_tab, int s0, int s1_) {
        seg_row0 = row0_tab, seg_rows = rows_tab, s1 = s1_;
        seg_at(s0);
    }
    __device__ __forceinline__ void seg_at(int sg_) {
        sg = sg_;
        row0 = __builtin_amdgcn_readfirstlane(seg_row0[sg]);
        nrows = __builtin_amdgcn_readfirstlane(seg_rows[sg]);
        nblk = (nrows + 15) >> 4;
        blk = 0, hs = 0;
    }
    __device__ __forceinline__ void advance(int tpb) {
        if (hs + 1 < tpb) {
            hs += 1;
        } else if (blk + 1 < nblk) {
            blk += 1, hs = 0;
        } else if (sg + 1 < s1) {
            seg_at(sg + 1);
        } else {
            blk = nblk;
        }
    }
};

// launch-site dispatch of the fused forms: f(integral_constant<int, gram>{}, bool_constant<nt>{}) for gram in {0, 1, 2}
// (mcl_launch_contract_xc) and nt = non-temporal loads of X (x_streams)
template <class F>
static inline int xc_gram_dispatch(int gram, bool nt, F &&f) {
    auto with_nt = [&](auto gram_c) { return nt ? f(gram_c, std::true_type{}) : f(gram_c, std::false_type{}); };
    if (gram == 2) return with_nt(std::integral_constant<int, 2>{});
    if (gram == 1) return with_nt(std::integral_constant<int, 1>{});
    return with_nt(std::integral_constant<int, 0>{});
}
