// inter_cost.hip — fused inter candidate evaluation: per job one 2Nx2N CU against up to K candidate
// motions (merge candidates, the two bidir estimates, or one plain motion compensation), as SA8D
// distortions, calcRdSADCost and the winner with its prediction (x265amd_inter_costs).
//
// Reference semantics: x265_1.9/source
//   encoder/analysis.cpp  checkMerge2Nx2N_rd0_4 :1652-1766 (the candidate loop :1689-1724)
//                         checkBidir2Nx2N       :2013-2140
//   common/predict.cpp    predInterLumaPixel :251-272   predInterLumaShort :274-305
//                         predInterChromaPixel :307-355 predInterChromaShort :357-407
//   common/ipfilter.cpp   the eight filter forms :40-372      common/pixel.cpp  addAvg :789-808, sa8d :244-322
//
// Work mapping: one wavefront per workgroup, a CU owned by G = (N/8)^2 lanes of it (64 / 16 / 4 / 1
// lanes for 64x64 / 32x32 / 16x16 / 8x8, so 1 / 4 / 16 / 64 CUs per wave), one 8x8 luma sub-block per
// lane.  The CU's candidates run one after the other in its lanes: the distortion total is then in
// every lane of the group when the candidate ends, the decision needs no exchange, the LDS footprint
// does not grow with K, and the best candidate's prediction so far stays in the lanes' registers (48 of
// them) until it is stored after the decision.  Per candidate and list the group stages the reference window —
// N rows, N + 7 when the MV has a vertical fraction; N columns, N + 7 with a horizontal one: exactly
// the reference's footprint — into LDS, runs the horizontal pass over it into an int16 LDS image
// (row-extended when a vertical pass follows), and each lane then runs the vertical pass of its
// sub-block into registers.  Uni rounds to pixels as the pp / sp forms do; bi keeps the int16 of the
// ps / ss forms of list 0 in registers and joins list 1 by addAvg.  The lane subtracts its source
// sub-block and runs the Hadamard of hadamard.h; sub-block sums meet by shuffles at the reference's
// rounding granularity.  Chroma reuses the same body with the 4-tap table at half size, Cb and Cr
// side by side in the lanes' lower half (8x8 CU: both 4x4 blocks in the one lane, SATD form).
// Nothing but sad / cost / best and the winner's prediction reaches global memory.
#include "common.h"
#include "../../../include/x265_amd.h"

namespace x265amd {

#include "hadamard.h"

struct InterCostArgs
{
    int n, K, depth;
    int fenc_stride, ref_stride, fenc_cstride, ref_cstride, pred_stride, pred_cstride;   // validated to fit
    const void* fenc; const int64_t* fenc_off;
    const void* ref;  const int64_t* ref_off;
    const uint8_t* dir;
    const int16_t* mv;
    const uint32_t* bits;
    const uint32_t* lambda;
    const void* fenc_cb; const void* fenc_cr; const int64_t* fenc_coff;
    const void* ref_cb;  const void* ref_cr;  const int64_t* ref_coff;
    uint32_t* sad;
    uint64_t* cost;
    x265amd_inter_best* best;
    void* pred; const int64_t* pred_off;
    void* pred_cb; void* pred_cr; const int64_t* pred_coff;
};

constexpr int kInterCostWave = 64;

// lanes per CU
constexpr int inter_cost_lanes(int N) { return (N / 8) * (N / 8); }

// LDS images of one plane set: the reference window W and the int16 result H of the horizontal pass,
// both in a frame shifted by HT rows and 4 columns (so a row piece starts 8-byte aligned) with one
// row stride S (4 mod 8 elements from 16x16 on); H follows W at SZ
template <int D, int TAPS>
struct McGeom
{
    static constexpr int HT = TAPS / 2 - 1, TA = TAPS / 2, ROWS = D + TAPS - 1, S = D + (D <= 8 ? 8 : 12);
    static constexpr int SZ = ROWS * S;
};

// one list of a candidate: element offset of the block at the MV's integer part, and the fractions
struct McList
{
    int64_t off;
    int fx, fy;
};

// the filter of coeffIdx idx as TAPS / 2 packed pairs (c[2m], c[2m + 1]), the form v_dot2_i32_i16 takes
template <int TAPS>
__device__ __forceinline__ void load_taps(int idx, s16x2 (&c)[TAPS / 2])
{
    if constexpr (TAPS == 8)
    {
        const uint4 v = ldu<uint4>(&c_luma.c[idx & 3][0]);
        c[0] = __builtin_bit_cast(s16x2, v.x); c[1] = __builtin_bit_cast(s16x2, v.y);
        c[2] = __builtin_bit_cast(s16x2, v.z); c[3] = __builtin_bit_cast(s16x2, v.w);
    }
    else
    {
        const uint2 v = ldu<uint2>(&c_chroma.c[idx & 7][0]);
        c[0] = __builtin_bit_cast(s16x2, v.x); c[1] = __builtin_bit_cast(s16x2, v.y);
    }
}

// 2 CW 16-bit values at an 8-byte aligned LDS address, as CW packed pairs of neighbours
template <int CW>
__device__ __forceinline__ void lds_read_pk(const uint16_t* p, uint32_t (&o)[CW])
{
#pragma unroll
    for (int i = 0; i < CW / 2; i++)
    {
        const uint2 v = *(const uint2*)(p + 4 * i);
        o[2 * i] = v.x; o[2 * i + 1] = v.y;
    }
}

// CW 16-bit values at an 8-byte aligned LDS address, sign-extended (pixels stay below 1 << 12)
template <int CW>
__device__ __forceinline__ void lds_read16(const uint16_t* p, int (&o)[CW])
{
#pragma unroll
    for (int i = 0; i < CW / 4; i++)
    {
        const uint2 v = *(const uint2*)(p + 4 * i);
        o[4 * i] = (int16_t)(v.x & 0xffff); o[4 * i + 1] = (int16_t)(v.x >> 16);
        o[4 * i + 2] = (int16_t)(v.y & 0xffff); o[4 * i + 3] = (int16_t)(v.y >> 16);
    }
}

template <int CW>
__device__ __forceinline__ void lds_write16(uint16_t* p, const int (&v)[CW])
{
#pragma unroll
    for (int i = 0; i < CW / 4; i++)
    {
        uint2 w;
        w.x = (uint32_t)(v[4 * i] & 0xffff) | ((uint32_t)v[4 * i + 1] << 16);
        w.y = (uint32_t)(v[4 * i + 2] & 0xffff) | ((uint32_t)v[4 * i + 3] << 16);
        *(uint2*)(p + 4 * i) = w;
    }
}

// Motion compensation and distortion of NPL planes of D x D (luma: one plane, 8 taps; chroma: Cb and
// Cr, 4 taps) for one candidate, in the G lanes of a CU; sub-blocks of B x B, lane g owns sub-block
// g (+ G, for the two 4x4 of an 8x8 CU's single lane).  Leaves the lane's part of the prediction in v
// (rows 2k, 2k + 1 paired) and returns the planes' sa8d, summed over the group at the reference's
// rounding granularity.
template <typename P, int TAPS, int D, int B, int NPL, int G, int SZ>
__device__ __forceinline__ uint32_t mc_planes(uint16_t* L, int g, int dir, McList l0, McList l1,
                                              const P* ref0, const P* ref1, int rs, const P* fenc0,
                                              const P* fenc1, int fs, int depth,
                                              s16x2 (&v)[(NPL * (D / B) * (D / B) + G - 1) / G][B / 2][B])
{
    typedef McGeom<D, TAPS> Geo;
    constexpr int HT = Geo::HT, TA = Geo::TA, ROWS = Geo::ROWS, S = Geo::S;
    constexpr int NB = D / B, SUBS = NB * NB, NSUB = NPL * SUBS, NSL = (NSUB + G - 1) / G;
    constexpr int CH = D / B;                              // row pieces of B pixels
    constexpr int LCH = CH == 1 ? 0 : CH == 2 ? 1 : CH == 4 ? 2 : 3, LPL = NPL - 1;
    static_assert(NSUB <= G || G == 1, "more than one sub-block per lane only in the one-lane form");
    static_assert(NPL == 1 || NPL == 2, "one plane or a chroma pair");
    static_assert(NPL * Geo::SZ <= SZ, "the plane set fits the images");
    // the lane's coordinates are re-derived per call from an opaque copy of g, so that the compiler does not
    // hoist the per-lane row addresses of every phase out of the candidate loop and keep them all live
    asm volatile("" : "+v"(g));
    // (plain values, not the two structs picked by l: a pointer select would put them in scratch)
    const int64_t off0 = l0.off, off1 = l1.off;
    const int fx0 = l0.fx, fx1 = l1.fx, fy0 = l0.fy, fy1 = l1.fy;
    uint16_t* const W = L;
    uint16_t* const H = L + SZ;

    const bool bi = dir == 3;
    const int maxv = (1 << depth) - 1;
    const int hr = 14 - depth;                             // IF_INTERNAL_PREC - depth
    const int ps_shift = 6 - hr, ps_off = -(8192 << ps_shift);

#pragma unroll 1
    for (int l = 0; l < 2; l++)
    {
        if (!((dir >> l) & 1)) continue;
        const int64_t off = l ? off1 : off0;
        const int fx = l ? fx1 : fx0, fy = l ? fy1 : fy0;
        const bool first = bi && l == 0;
        const int nrows = D + (fy ? TAPS - 1 : 0), r0 = fy ? 0 : HT;     // staged rows, in the shifted frame

        // ---- stage the window: N columns in pieces of B, and the 3 + 4 (1 + 2) beside them only when the
        // MV has a horizontal fraction.  Four items per lane and trip, their loads issued together; an index
        // past the end repeats the last item (the same data to the same place) instead of branching.
        constexpr int U = 4;
        {
            const int items = nrows * NPL * CH;
            for (int it0 = g; it0 < items; it0 += U * G)
            {
                int px[U][B], wo[U];
#pragma unroll
                for (int u = 0; u < U; u++)
                {
                    const int it = min(it0 + u * G, items - 1);
                    const int c = it & (CH - 1), pl = (it >> LCH) & LPL, rr = r0 + (it >> (LCH + LPL));
                    load_row<P, B>((pl ? ref1 : ref0) + off + (int64_t)(rr - HT) * rs + c * B, px[u]);
                    wo[u] = (pl * ROWS + rr) * S + 4 + c * B;
                }
#pragma unroll
                for (int u = 0; u < U; u++) lds_write16<B>(W + wo[u], px[u]);
            }
        }
        if (fx)
        {
            // HT + 1 = TA pixels on either side: the left piece carries column 0 along (inside the footprint,
            // and the value the body wrote there)
            static_assert(HT + 1 == TA, "the two side pieces have one width");
            const int items = nrows * NPL * 2;
            for (int it0 = g; it0 < items; it0 += U * G)
            {
                int px[U][TA], wo[U];
#pragma unroll
                for (int u = 0; u < U; u++)
                {
                    const int it = min(it0 + u * G, items - 1);
                    const int c0 = (it & 1) ? D : -HT, pl = (it >> 1) & LPL, rr = r0 + (it >> (1 + LPL));
                    load_row<P, TA>((pl ? ref1 : ref0) + off + (int64_t)(rr - HT) * rs + c0, px[u]);
                    wo[u] = (pl * ROWS + rr) * S + 4 + c0;
                }
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int e = 0; e < TA; e++) W[wo[u] + e] = (uint16_t)px[u][e];
            }
        }
        wave_sync();

        // ---- horizontal pass into H: hpp when nothing follows it (uni, no vertical fraction), else hps
        if (fx)
        {
            s16x2 cf[TAPS / 2];
            load_taps<TAPS>(fx, cf);
            const bool pp = !bi && !fy;
            const int items = nrows * NPL * CH;
            for (int it0 = g; it0 < items; it0 += 2 * G)
#pragma unroll
            for (int u = 0; u < 2; u++)               // two independent items per trip (past the end: the last one again)
            {
                const int it = min(it0 + u * G, items - 1);
                const int c = it & (CH - 1), pl = (it >> LCH) & LPL, rr = r0 + (it >> (LCH + LPL));
                uint32_t A[(B + 8) / 2];                   // columns c B - 4 .. c B + B + 3, as pairs of neighbours
                lds_read_pk<(B + 8) / 2>(W + (pl * ROWS + rr) * S + c * B, A);
                int o[B];
#pragma unroll
                for (int x = 0; x < B; x++)
                {
                    // v_dot2_i32_i16 over the pairs of the window (odd starts: the pair straddling two registers)
                    int sum = 0;
#pragma unroll
                    for (int m = 0; m < TAPS / 2; m++)
                    {
                        const int e = 4 - HT + x + 2 * m;
                        const uint32_t pr = (e & 1) ? __builtin_amdgcn_alignbit(A[(e + 1) / 2], A[(e - 1) / 2], 16) : A[e / 2];
                        sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr), cf[m], sum, false);
                    }
                    if (pp)
                    {
                        const int q = (int16_t)((sum + 32) >> 6);
                        o[x] = q < 0 ? 0 : (q > maxv ? maxv : q);
                    }
                    else
                        o[x] = (int16_t)((sum + ps_off) >> ps_shift);
                }
                lds_write16<B>(H + (pl * ROWS + rr) * S + 4 + c * B, o);
            }
            wave_sync();
        }

        // ---- the lane's sub-block(s): vertical pass, or the rows as they are
        s16x2 cv[TAPS / 2];
        load_taps<TAPS>(fy, cv);
        // rounding of the vertical forms: vsp / vss after a horizontal pass, vpp / vps on pixels
        const int vsh = fx ? (bi ? 6 : 6 + hr) : (bi ? ps_shift : 6);
        const int voff = fx ? (bi ? 0 : (1 << (5 + hr)) + (8192 << 6)) : (bi ? ps_off : 32);
        const int ashift = hr + 1, aoff = (1 << hr) + 2 * 8192;           // addAvg
#pragma unroll
        for (int q = 0; q < NSL; q++)
        {
            const int sb = g + q * G;
            if (sb >= NSUB) continue;
            const int pl = sb / SUBS, s = sb % SUBS;
            const int X0 = ((s & 1) | ((s >> 1) & 2) | ((s >> 2) & 4)) * B;
            const int Y0 = (((s >> 1) & 1) | ((s >> 2) & 2) | ((s >> 3) & 4)) * B;
            const uint16_t* sp = (fx ? H : W) + (pl * ROWS + Y0) * S + 4 + X0;        // rows at immediate offsets
            int val[B][B];
            if (fy)
            {
#pragma unroll
                for (int y = 0; y < B; y++)
#pragma unroll
                    for (int x = 0; x < B; x++) val[y][x] = 0;
                // rows j, j + 1 paired per column (v_perm), one v_dot2_i32_i16 per two taps, scattered to the outputs
                uint32_t prev[B / 2];
                lds_read_pk<B / 2>(sp, prev);
#pragma unroll
                for (int j = 0; j < B + TAPS - 2; j++)
                {
                    uint32_t cur[B / 2];
                    lds_read_pk<B / 2>(sp + (j + 1) * S, cur);
#pragma unroll
                    for (int h = 0; h < B / 2; h++)
                    {
                        const s16x2 lo = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(cur[h], prev[h], 0x05040100u));
                        const s16x2 hi = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(cur[h], prev[h], 0x07060302u));
#pragma unroll
                        for (int m = 0; m < TAPS / 2; m++)
                        {
                            const int y = j - 2 * m;
                            if (y < 0 || y >= B) continue;
                            val[y][2 * h] = __builtin_amdgcn_sdot2(lo, cv[m], val[y][2 * h], false);
                            val[y][2 * h + 1] = __builtin_amdgcn_sdot2(hi, cv[m], val[y][2 * h + 1], false);
                        }
                        prev[h] = cur[h];
                    }
                }
#pragma unroll
                for (int y = 0; y < B; y++)
#pragma unroll
                    for (int x = 0; x < B; x++)
                    {
                        const int o = (int16_t)((val[y][x] + voff) >> vsh);
                        val[y][x] = bi ? o : (o < 0 ? 0 : (o > maxv ? maxv : o));
                    }
            }
            else
            {
#pragma unroll
                for (int y = 0; y < B; y++)
                {
                    int in[B];
                    lds_read16<B>(sp + (HT + y) * S, in);
#pragma unroll
                    for (int x = 0; x < B; x++)
                        val[y][x] = (fx || !bi) ? in[x] : (int)(int16_t)(in[x] << hr) - 8192;   // hpp / hps / copy, p2s
                }
            }
#pragma unroll
            for (int k = 0; k < B / 2; k++)
#pragma unroll
                for (int x = 0; x < B; x++)
                {
                    int o0 = val[2 * k][x], o1 = val[2 * k + 1][x];
                    if (bi && !first)
                    {
                        o0 = ((int)v[q][k][x].x + o0 + aoff) >> ashift;
                        o1 = ((int)v[q][k][x].y + o1 + aoff) >> ashift;
                        o0 = o0 < 0 ? 0 : (o0 > maxv ? maxv : o0);
                        o1 = o1 < 0 ? 0 : (o1 > maxv ? maxv : o1);
                    }
                    v[q][k][x] = s16x2{(short)o0, (short)o1};
                }
        }
        wave_sync();                                       // the next list (or plane set) restages W and H
    }

    // ---- the Hadamard of the difference to the source
    uint32_t r = 0;
#pragma unroll
    for (int q = 0; q < NSL; q++)
    {
        const int sb = g + q * G;
        if (sb >= NSUB) continue;
        const int pl = sb / SUBS, s = sb % SUBS;
        const int X0 = ((s & 1) | ((s >> 1) & 2) | ((s >> 2) & 4)) * B;
        const int Y0 = (((s >> 1) & 1) | ((s >> 2) & 2) | ((s >> 3) & 4)) * B;
        const P* f = (pl ? fenc1 : fenc0) + (int64_t)Y0 * fs + X0;
        constexpr bool PK = sizeof(P) == 1 && B == 8;       // packed 16-bit Hadamard (8-bit pixels)
        int d[PK ? 1 : B][PK ? 1 : B];
        s16x2 Q[PK ? 4 : 1][PK ? 8 : 1];
#pragma unroll
        for (int k = 0; k < B / 2; k++)
        {
            int f0[B], f1[B];
            load_row<P, B>(f + (int64_t)(2 * k) * fs, f0);
            load_row<P, B>(f + (int64_t)(2 * k + 1) * fs, f1);
#pragma unroll
            for (int x = 0; x < B; x++)
            {
                if constexpr (PK) Q[k][x] = s16x2{(short)f0[x], (short)f1[x]} - v[q][k][x];
                else { d[2 * k][x] = f0[x] - (int)v[q][k][x].x; d[2 * k + 1][x] = f1[x] - (int)v[q][k][x].y; }
            }
        }
        uint32_t raw;
        if constexpr (B == 4) raw = had4x4_raw(d);
        else if constexpr (PK) raw = had8x8_pk(Q);
        else raw = had8x8(d);
        // 4x4: satd_4x4; 8x8: sa8d_8x8, rounded alone; from 16x16 on the four 8x8 of a 16x16 round together
        r += D == 4 ? raw >> 1 : D == 8 ? (raw + 2) >> 2 : raw;
    }
    if constexpr (D >= 16)
    {
        r += __shfl_xor(r, 1, 64);
        r += __shfl_xor(r, 2, 64);
        r = (g & 3) ? 0 : (r + 2) >> 2;
    }
    return group_sum<G>(r);
}

// the lanes' sub-blocks of a prediction (rows paired as mc_planes leaves them) to the CU's place in pred
template <typename P, int D, int B, int NPL, int G>
__device__ __forceinline__ void store_planes(const s16x2 (&v)[(NPL * (D / B) * (D / B) + G - 1) / G][B / 2][B], int g,
                                             P* pred0, P* pred1, int ps)
{
    constexpr int SUBS = (D / B) * (D / B), NSUB = NPL * SUBS, NSL = (NSUB + G - 1) / G;
#pragma unroll
    for (int q = 0; q < NSL; q++)
    {
        const int sb = g + q * G;
        if (sb >= NSUB) continue;
        const int pl = sb / SUBS, s = sb % SUBS;
        const int X0 = ((s & 1) | ((s >> 1) & 2) | ((s >> 2) & 4)) * B;
        const int Y0 = (((s >> 1) & 1) | ((s >> 2) & 2) | ((s >> 3) & 4)) * B;
        P* d = (pl ? pred1 : pred0) + (int64_t)Y0 * ps + X0;
#pragma unroll
        for (int k = 0; k < B / 2; k++)
        {
            int r0[B], r1[B];
#pragma unroll
            for (int x = 0; x < B; x++) { r0[x] = v[q][k][x].x; r1[x] = v[q][k][x].y; }
            store_row<P, B>(d + (int64_t)(2 * k) * ps, r0);
            store_row<P, B>(d + (int64_t)(2 * k + 1) * ps, r1);
        }
    }
}

template <typename P, int N>
__global__ __launch_bounds__(kInterCostWave) void k_inter_costs(const InterCostArgs a)
{
    constexpr int G = inter_cost_lanes(N), JOBS = kInterCostWave / G, M = N / 2, CB = N == 8 ? 4 : 8;
    constexpr int SZ = McGeom<N, 8>::SZ;
    static_assert(SZ % 4 == 0, "8-byte aligned images");
    __shared__ __attribute__((aligned(16))) uint16_t L[JOBS][2 * SZ];    // per CU: W, then H

    const int t = threadIdx.x, slot = t / G, g = t % G;
    const int64_t job = (int64_t)xcd_block() * JOBS + slot;
    if (job >= a.n) return;                                // whole groups leave: the kernel has no hardware barrier

    const int K = a.K;
    const bool rd = a.bits != nullptr;
    const bool chroma = a.ref_cb != nullptr;
    const uint64_t lam = rd ? a.lambda[job] : 0;
    const P* const fe = (const P*)a.fenc + a.fenc_off[job];
    P* const pd = a.pred ? (P*)a.pred + a.pred_off[job] : nullptr;
    const int64_t fco = chroma ? a.fenc_coff[job] : 0, pco = a.pred_cb ? a.pred_coff[job] : 0;
    const P* const fcb = (const P*)a.fenc_cb + fco;
    const P* const fcr = (const P*)a.fenc_cr + fco;
    P* const pcb = (P*)a.pred_cb + pco;
    P* const pcr = (P*)a.pred_cr + pco;
    const bool wpred = pd != nullptr, wpredc = a.pred_cb != nullptr;

    typedef const __attribute__((address_space(4))) InterCostArgs* KArgs;   // the kernel's argument, in the kernarg segment
    uint64_t bc = (uint64_t)INT64_MAX;
    int bk = -1;
    uint32_t bsad = 0, bbits = 0;
    // the candidates in slot order; the best one's prediction so far stays in registers (rows paired, 32 + 16
    // registers) and is stored once after the decision
    constexpr int NSLC = (2 * (M / CB) * (M / CB) + G - 1) / G;
    s16x2 vl[1][4][8], vc[NSLC][CB / 2][CB], bl[1][4][8], bcr[NSLC][CB / 2][CB];
#pragma unroll 1
    for (int k = 0; k < K; k++)
    {
        // the arguments a candidate needs are read from the kernarg segment where they are used (through a pointer
        // the compiler cannot see through), not held in scalar registers across the whole loop
        KArgs q = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(q));
        const int64_t ck = job * K + k;
        const int dir = q->dir[ck] & 3;
        if (dir == 0)
        {
            if (g == 0)
            {
                if (q->sad) q->sad[ck] = 0xFFFFFFFFu;
                if (q->cost) q->cost[ck] = ~(uint64_t)0;
            }
            continue;
        }
        // (four separate objects, not arrays: a list picked by a run-time index would put them in scratch)
        McList ll0, ll1, lc0, lc1;
        {
            const int16_t* mv = q->mv + ck * 4;
            const int x0 = mv[0], y0 = mv[1], x1 = mv[2], y1 = mv[3];
            ll0.off = q->ref_off[ck * 2] + (int64_t)(y0 >> 2) * q->ref_stride + (x0 >> 2);
            ll1.off = q->ref_off[ck * 2 + 1] + (int64_t)(y1 >> 2) * q->ref_stride + (x1 >> 2);
            ll0.fx = x0 & 3; ll0.fy = y0 & 3; ll1.fx = x1 & 3; ll1.fy = y1 & 3;
            lc0.off = (chroma ? q->ref_coff[ck * 2] : 0) + (int64_t)(y0 >> 3) * q->ref_cstride + (x0 >> 3);
            lc1.off = (chroma ? q->ref_coff[ck * 2 + 1] : 0) + (int64_t)(y1 >> 3) * q->ref_cstride + (x1 >> 3);
            lc0.fx = x0 & 7; lc0.fy = y0 & 7; lc1.fx = x1 & 7; lc1.fy = y1 & 7;
        }
        uint32_t sad = mc_planes<P, 8, N, 8, 1, G, SZ>(L[slot], g, dir, ll0, ll1, (const P*)q->ref, (const P*)q->ref,
                                                       q->ref_stride, fe, fe, q->fenc_stride, q->depth, vl);
        if (chroma)
            sad += mc_planes<P, 4, M, CB, 2, G, SZ>(L[slot], g, dir, lc0, lc1, (const P*)q->ref_cb, (const P*)q->ref_cr,
                                                    q->ref_cstride, fcb, fcr, q->fenc_cstride, q->depth, vc);
        asm volatile("" : "+s"(q));
        const uint32_t b = rd ? q->bits[ck] : 0;
        const uint64_t c = (uint64_t)sad + (((uint64_t)b * lam + 128) >> 8);
        if (g == 0)
        {
            if (q->sad) q->sad[ck] = sad;
            if (q->cost) q->cost[ck] = c;
        }
        if (c < bc)                                        // strict <: the first minimum in slot order
        {
            bc = c; bk = k; bsad = sad; bbits = b;
            if (wpred)
            {
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int x = 0; x < 8; x++) bl[0][i][x] = vl[0][i][x];
                if (wpredc)
                {
#pragma unroll
                    for (int s = 0; s < NSLC; s++)
#pragma unroll
                        for (int i = 0; i < CB / 2; i++)
#pragma unroll
                            for (int x = 0; x < CB; x++) bcr[s][i][x] = vc[s][i][x];
                }
            }
        }
    }
    if (wpred && bk >= 0)
    {
        store_planes<P, N, 8, 1, G>(bl, g, pd, pd, a.pred_stride);
        if (wpredc) store_planes<P, M, CB, 2, G>(bcr, g, pcb, pcr, a.pred_cstride);
    }
    if (a.best && g == 0)
    {
        x265amd_inter_best o;
        o.cost = bc;
        o.sad = bsad;
        o.bits = bbits;
        o.cand = bk;
        o.reserved = 0;
        a.best[job] = o;
    }
}

template <typename P, int N>
static int launch_inter(const InterCostArgs& a, hipStream_t st)
{
    constexpr int JOBS = kInterCostWave / inter_cost_lanes(N);
    const dim3 grid((uint32_t)((a.n + JOBS - 1) / JOBS));
    hipLaunchKernelGGL((k_inter_costs<P, N>), grid, dim3(kInterCostWave), 0, st, a);
    return (int)hipGetLastError();
}

template <typename P>
static int launch_inter_size(int log2_size, const InterCostArgs& a, hipStream_t st)
{
    switch (log2_size)
    {
    case 3: return launch_inter<P, 8>(a, st);
    case 4: return launch_inter<P, 16>(a, st);
    case 5: return launch_inter<P, 32>(a, st);
    case 6: return launch_inter<P, 64>(a, st);
    }
    return X265AMD_EINVAL;
}

} // namespace x265amd

using namespace x265amd;

extern "C" int x265amd_inter_costs(int depth, int count, const x265amd_inter_cost_batch* bt, void* stream)
{
    if (depth != 8 && depth != 10 && depth != 12) return X265AMD_EINVAL;
    if (count < 0 || (count && !bt)) return X265AMD_EINVAL;
    // validate every batch before enqueuing anything
    for (int i = 0; i < count; i++)
    {
        const x265amd_inter_cost_batch& b = bt[i];
        if (b.n < 0) return X265AMD_EINVAL;
        if (!b.n) continue;                                // an empty batch is a no-op, whatever else it holds
        if (b.log2_size < 3 || b.log2_size > 6) return X265AMD_EINVAL;
        if (b.max_cand < 1 || b.max_cand > 5) return X265AMD_EINVAL;
        if (!b.fenc || !b.fenc_off || !b.ref || !b.ref_off || !b.dir || !b.mv) return X265AMD_EINVAL;
        const int nc = !!b.fenc_cb + !!b.fenc_cr + !!b.fenc_coff + !!b.ref_cb + !!b.ref_cr + !!b.ref_coff;
        if (nc != 0 && nc != 6) return X265AMD_EINVAL;
        const int np = !!b.pred_cb + !!b.pred_cr + !!b.pred_coff;
        if (np != 0 && np != 3) return X265AMD_EINVAL;
        if (np && (!nc || !b.pred)) return X265AMD_EINVAL;
        if (b.pred && !b.pred_off) return X265AMD_EINVAL;
        if ((b.cost || b.best || b.pred) && (!b.bits || !b.lambda)) return X265AMD_EINVAL;
        if (!b.sad && !b.cost && !b.best && !b.pred) return X265AMD_EINVAL;
        // strides travel as 32-bit values
        const intptr_t st[6] = { b.fenc_stride, b.ref_stride, nc ? b.fenc_cstride : 0, nc ? b.ref_cstride : 0,
                                 b.pred ? b.pred_stride : 0, np ? b.pred_cstride : 0 };
        for (int k = 0; k < 6; k++)
            if (st[k] != (intptr_t)(int)st[k]) return X265AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++)
    {
        const x265amd_inter_cost_batch& b = bt[i];
        if (!b.n) continue;
        InterCostArgs a;
        a.n = b.n; a.K = b.max_cand; a.depth = depth;
        a.fenc = b.fenc; a.fenc_stride = (int)b.fenc_stride; a.fenc_off = b.fenc_off;
        a.ref = b.ref; a.ref_stride = (int)b.ref_stride; a.ref_off = b.ref_off;
        a.dir = b.dir; a.mv = b.mv;
        // the bits only enter cost / best: without both of them the kernel writes distortions only
        const bool rd = b.bits && b.lambda;
        a.bits = rd ? b.bits : nullptr; a.lambda = b.lambda;
        a.fenc_cb = b.fenc_cb; a.fenc_cr = b.fenc_cr; a.fenc_cstride = (int)b.fenc_cstride; a.fenc_coff = b.fenc_coff;
        a.ref_cb = b.ref_cb; a.ref_cr = b.ref_cr; a.ref_cstride = (int)b.ref_cstride; a.ref_coff = b.ref_coff;
        a.sad = b.sad; a.cost = b.cost; a.best = b.best;
        a.pred = b.pred; a.pred_stride = (int)b.pred_stride; a.pred_off = b.pred_off;
        a.pred_cb = b.pred_cb; a.pred_cr = b.pred_cr; a.pred_cstride = (int)b.pred_cstride; a.pred_coff = b.pred_coff;
        const int rc = depth == 8 ? launch_inter_size<uint8_t>(b.log2_size, a, st)
                                  : launch_inter_size<uint16_t>(b.log2_size, a, st);
        if (rc) return rc;
    }
    return 0;
}
