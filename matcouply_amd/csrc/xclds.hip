// k_contract_xc_lds : XC = X C for K % 512 == 0 with the WHOLE fragment image of C resident in LDS (K x 16 NB floats <= 128 KB).
//
// k_contract_xc_row (contract.hip) re-reads the C fragments of every 256-column super-chunk from L2 into 64 NB registers, and
// because memory returns in order those loads have to be issued BEFORE the prefetch of the next X tile and waited for in front of
// it: one tile (16 KB per wave) is all a wave ever has in flight, at 492 VGPRs a SIMD holds one wave, and at config 5 (K = 1024,
// rank 32) the pass waits for memory half of its life (profiles/r6_c5_sq_counters.json: SQ_WAIT_INST_ANY 52 % of SQ_WAVE_CYCLES)
// and moves 70.9 GB in 16.7 ms = 4.4 TB/s where a streaming read reaches 6.8.  Here
//   * the workgroup copies the fragment image of C into LDS once (config 5: 128 KB of the CU's 160 KB; the MFMA B operands are
//     16-byte LDS reads, lane-linear: conflict-free; cfrag_at on the LDS base),
//   * so the ONLY loads of the main loop are the X tiles (and, once per round, the rows of B for the fused A-phase reductions, in
//     the same batch): a DEPTH-slot register ring keeps four or eight 16-row x 128-column tiles (32 / 64 KB per wave) in
//     flight under exact s_waitcnt vmcnt(N) counts - every load unconditional at clamped addresses, a fixed number per step,
//   * tiles are staged through a wave-private 8 KB XcTile<128>.
// What is not the pipeline comes from xc_parts.h: the tile, the walk (SegCursor with K / 128 tiles per block), the four fp32
// chains per output (one per 64-column chunk modulo 4, ascending in K) and their sum (chains_sum4), the rows of B
// (b_rows_clamped) and the fused reductions (SegGram).  Same segment / wave tables as k_contract_xc_row.
#include "mcl_internal.h"
#include "xc_parts.h"
#include "xload.h"

namespace {

template <class XL, int NB, int GRAM, bool XNT, int DEPTH>
static __device__ __forceinline__ void k_contract_xc_lds_body(const typename XL::T *X, const float *Cfrag, float *XC, const float *B, const int *seg_row0, const int *seg_rows, const int *wave_seg_ptr, int n_waves, int K, int r, double *seg_rhs, double *seg_btb) {
    extern __shared__ float lds_dyn[];  // fragment image of C, then 4 waves x 16 rows x 128 floats
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, i16 = lane & 15;
    const int cf_f4 = (K >> 6) * 4 * NB * 64;  // float4 elements of the image
    {
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds_dyn);
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Cfrag);
        for (int e = threadIdx.x; e < cf_f4; e += 256) dst[e] = src[e];
    }
    __syncthreads();
    using Tile = XcTile<128>;
    float *L = lds_dyn + 4 * cf_f4 + wave * (16 * 128);
    const int w = blockIdx.x * 4 + wave;
    if (w >= n_waves) return;
    const int s0 = wave_seg_ptr[w], s1 = wave_seg_ptr[w + 1];
    if (s0 >= s1) return;
    const int TPB = K >> 7;  // tiles per 16-row block (a multiple of DEPTH)

    // ---- the prefetch side: DEPTH tiles in registers
    typename XL::raw xr[DEPTH][8];
    float bnx[NB][4];  // rows 4q + v, column 16 nb + i16 of B for the block the prefetch cursor is in
    int bcolc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bcolc[nb] = min(16 * nb + i16, r - 1);
    const int half = lane >> 5, slot = lane & 31;
    auto issue = [&](const SegCursor &c, typename XL::raw (&dst)[8]) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const long j = c.row0 + min(16 * c.blk + 2 * t + half, c.nrows - 1);
            dst[t] = XL::template ld4<XNT>(X + j * K + 128 * c.hs + 4 * slot);
        }
    };
    auto issue_b = [&](const SegCursor &c) {
        if (GRAM) b_rows_clamped<NB>(B, c.row0, c.blk, c.nrows, r, bcolc, q, bnx);
    };

    SegCursor pc;  // prefetch cursor
    pc.begin(seg_row0, seg_rows, s0, s1);
    SegCursor cc = pc;  // compute cursor: stepped by hand below, the epilogues sit between its steps
    issue_b(pc);
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
        issue(pc, xr[s]);
        pc.advance(TPB);
    }

    long total_rounds = 0;
    for (int sg = s0; sg < s1; ++sg) total_rounds += (long)((__builtin_amdgcn_readfirstlane(seg_rows[sg]) + 15) >> 4) * (TPB / DEPTH);

    constexpr int NCH = (NB == 4) ? 1 : 4;
    f32x4 acc4[NCH][NB];
#pragma unroll
    for (int kc = 0; kc < NCH; ++kc)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc4[kc][nb] = zero4();
    SegGram<NB, GRAM> gram;
    gram.reset();
    float bcur[NB][4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int v = 0; v < 4; ++v) bcur[nb][v] = 0.f;

    for (long rnd = 0; rnd < total_rounds; ++rnd) {
        if (GRAM && cc.hs == 0) {  // (wave-uniform; register moves only) the rows of B of the block that starts now
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int v = 0; v < 4; ++v) bcur[nb][v] = bnx[nb][v];
        }
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {
            // tile `cc` sits in xr[s]: registers -> LDS
#pragma unroll
            for (int t = 0; t < 8; ++t) Tile::put(L, 2 * t + half, slot, XL::cvt(xr[s][t]));
            // the slot is free: the tile DEPTH ahead (once per round with the rows of B of its block: a fixed number of loads)
            if (s == 0) issue_b(pc);
            issue(pc, xr[s]);
            pc.advance(TPB);
            __builtin_amdgcn_sched_barrier(0);
            const int chunk0 = 2 * cc.hs;  // 64-column chunks 2 hs, 2 hs + 1 of C
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                f32x4 fr[4];
#pragma unroll
                for (int kq = 0; kq < 4; ++kq) fr[kq] = Tile::frag(L, i16, q, kc, kq);
                f32x4 cf[4][NB];
#pragma unroll
                for (int kq = 0; kq < 4; ++kq)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) cf[kq][nb] = cfrag_at<NB>(lds_dyn, chunk0 + kc, kq, nb, lane);
                // the chain of chunk (2 hs + kc) mod 4: hs = s (mod 4) inside a round (DEPTH is a multiple of 4)
                const int ch = (NCH == 4) ? ((2 * s + kc) & 3) : 0;
#pragma unroll
                for (int kq = 0; kq < 4; ++kq)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) acc4[ch][nb] = MFMA16(fr[kq][m], cf[kq][nb][m], acc4[ch][nb]);
            }
            cc.hs += 1;
        }
        if (cc.hs < TPB) continue;
        // ---- end of the 16-row block
        f32x4 acc[NB];
        chains_sum4<NCH, NB>(acc4, acc);
        gram.block(acc, bcur, cc.row0, cc.blk, cc.nrows, r, XC, q, i16);
        cc.hs = 0;
        cc.blk += 1;
        if (cc.blk < cc.nblk) continue;
        // ---- end of the segment
        if (GRAM) {
            gram.store(cc.sg, r, seg_rhs, seg_btb, q, i16);
            gram.reset();
        }
        if (cc.sg + 1 < s1) cc.seg_at(cc.sg + 1);
    }
}
template <int NB, int GRAM, bool XNT, int DEPTH>
__global__ __launch_bounds__(256) void k_contract_xc_lds(const float *__restrict__ X, const float *__restrict__ Cfrag,
                                                         float *__restrict__ XC, const float *__restrict__ B,
                                                         const int *__restrict__ seg_row0, const int *__restrict__ seg_rows,
                                                         const int *__restrict__ wave_seg_ptr, int n_waves, int K, int r,
                                                         double *__restrict__ seg_rhs, double *__restrict__ seg_btb) {
    k_contract_xc_lds_body<XF32, NB, GRAM, XNT, DEPTH>(X, Cfrag, XC, B, seg_row0, seg_rows, wave_seg_ptr, n_waves, K, r, seg_rhs, seg_btb);
}
// the 16-bit twin (xload.h): the same template arguments after the element type
template <class XL, int NB, int GRAM, bool XNT, int DEPTH>
__global__ __launch_bounds__(256) void k_contract_xc_lds_h(const typename XL::T *__restrict__ X, const float *__restrict__ Cfrag,
                                                         float *__restrict__ XC, const float *__restrict__ B,
                                                         const int *__restrict__ seg_row0, const int *__restrict__ seg_rows,
                                                         const int *__restrict__ wave_seg_ptr, int n_waves, int K, int r,
                                                         double *__restrict__ seg_rhs, double *__restrict__ seg_btb) {
    k_contract_xc_lds_body<XL, NB, GRAM, XNT, DEPTH>(X, Cfrag, XC, B, seg_row0, seg_rows, wave_seg_ptr, n_waves, K, r, seg_rhs, seg_btb);
}

}  // namespace

// Launches the LDS-resident-C form of the X C pass when the shape allows it; returns 1 when launched, 0 otherwise.
// gram: 0 X C only, 1 fused per-segment reductions in fp32 chains, 2 in fp64.  MCL_XC_LDS_DEPTH=4 / 8 overrides the ring depth.
template <class XL>
static int try_xc_lds(mcl_context *c, int gram) {
    if (c->sw.no_xc_lds || c->NB > 2 || (c->K % 512) != 0 || (c->K % 4) != 0) return 0;
    if (!mcl_x_vec_aligned(c)) return 0;
    const size_t cf_bytes = (size_t)(c->K >> 6) * 4 * c->NB * 256 * sizeof(float);
    const size_t sm = cf_bytes + sizeof(float) * 4 * 16 * 128;
    if (sm > 160 * 1024) return 0;
    const int n_segs = c->segs.n_tiles;
    if (n_segs == 0) return 0;
    if (mcl_cfrag_chunks(c) != (int)(c->K >> 6)) return 0;  // (the image the kernel copies is exactly K / 64 chunks)
    const unsigned g = (unsigned)((c->n_seg_waves + 3) / 4);
    // tiles in flight per wave: four (32 KB).  Eight (MCL_XC_LDS_DEPTH=8, K % 1024 == 0) measured 13.68 against 13.39 ms at
    // config 5: with four the pass no longer waits for bytes in flight
    int depth = 4;
    if (c->sw.xc_lds_depth == 4 || c->sw.xc_lds_depth == 8) depth = (c->K % (128 * c->sw.xc_lds_depth) == 0) ? c->sw.xc_lds_depth : depth;
    constexpr bool F32 = std::is_same_v<XL, XF32>;  // (the depth-8 experiment has no 16-bit twin)
#define MCL_XCL__(NB_, GRAM_, NT_, D_)                                                                                    \
    do {                                                                                                                  \
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(MCL_XKERNEL(k_contract_xc_lds, NB_, GRAM_, NT_, D_)),       \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm) != hipSuccess) {                      \
            (void)hipGetLastError();                                                                                      \
            return 0;                                                                                                     \
        }                                                                                                                 \
        hipLaunchKernelGGL((MCL_XKERNEL(k_contract_xc_lds, NB_, GRAM_, NT_, D_)), dim3(g), dim3(256), sm, c->stream,          \
                           mcl_x<XL>(c), c->Cfrag,                                                                        \
                           c->XC, c->B, c->segs.row0, c->segs.nrows, c->wave_seg_ptr, c->n_seg_waves, (int)c->K, c->r,      \
                           c->seg_rhs, c->seg_btb);                                                                       \
    } while (0)
#define MCL_XCL_(NB_, GRAM_, NT_)                                \
    do {                                                         \
        if constexpr (F32) {                                     \
            if (depth == 8) MCL_XCL__(NB_, GRAM_, NT_, 8);       \
            else MCL_XCL__(NB_, GRAM_, NT_, 4);                  \
        } else {                                                 \
            MCL_XCL__(NB_, GRAM_, NT_, 4);                       \
        }                                                        \
    } while (0)
    auto launch = [&](auto nb_c) {
        return xc_gram_dispatch(gram, c->x_streams, [&](auto gram_c, auto nt_c) {
            constexpr int NB_ = decltype(nb_c)::value, GRAM_ = decltype(gram_c)::value;
            constexpr bool NT_ = decltype(nt_c)::value;
            MCL_XCL_(NB_, GRAM_, NT_);
            return hipGetLastError() == hipSuccess ? 1 : 0;
        });
    };
    return c->NB == 1 ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 2>{});
#undef MCL_XCL_
#undef MCL_XCL__
}

int mcl_try_contract_xc_lds(mcl_context *c, int gram) {
    return mcl_x_dispatch(c->x_type, [&](auto xl) { return try_xc_lds<decltype(xl)>(c, gram); });
}
