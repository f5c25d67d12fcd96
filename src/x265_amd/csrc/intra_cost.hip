// intra_cost.hip — fused intra mode decision: per job the 35 luma predictions of one PU against its
// source block, as SA8D costs plus the winning mode (x265amd_intra_costs).
//
// Reference semantics: x265_1.9/source/encoder/search.cpp
//   checkIntraInInter :1250-1343 + the full-search loop :1381-1388   estIntraPredQT :1488-1558
// with Predict::initAdiPattern(ALL_IDX) (predict.cpp:608-648: intraFilter or the strong bilinear
// smoothing at 32x32), scale2D_64to32 / scale1D_128to64 (pixel.cpp:504-547) for the 64x64 form,
// the predictors of intrapred.cpp and sa8d of pixel.cpp:244-322 (4x4: satd_4x4).
//
// Work mapping: one wavefront per workgroup, a job owned by G lanes of it (32 / 8 / 2 / 2 lanes for
// 32x32 / 16x16 / 8x8 / 4x4, so 2 / 8 / 32 / 32 jobs per wave).  The job's lanes read the source block
// and the 4N+1 neighbours once (the 64x64 form scales them while loading) into LDS, filter the
// neighbours there, and then split into two classes of G/2 lanes: class 0 works in the vertical
// frame (modes 18..34 and planar), class 1 in the flipped frame (modes 2..17 and DC; planar and DC
// are symmetric under the flip).  A lane keeps one 8x8 (4x4) sub-block of the source in registers —
// transposed for class 1, as SA8D is invariant under transposing both operands — and walks its
// class's 18 modes: per mode the class's lanes build the reference pairs D[j] = (R[j], R[j+1]) of
// intra.hip in LDS (projected left samples included), each lane predicts its sub-block from them
// (one ds_read_b32 + one v_dot2 per pixel), runs the Hadamard of hadamard.h on the difference and
// the sub-block sums meet by shuffles at the reference's rounding granularity.  The per-mode sums
// stay in LDS until the decision stage of the same kernel writes sad / cost / best: no prediction
// and no intermediate ever reaches global memory.
#include "common.h"
#include "intra_lane.h"
#include "../../../include/x265_amd.h"

namespace x265amd {

#include "hadamard.h"

struct IntraCostArgs
{
    int n, maxv, strong, threshold;
    const void* fenc;
    int64_t fenc_stride;
    const int64_t* fenc_off;
    const void* nb;
    const int64_t* nb_off;
    const uint8_t* mpm;
    const uint32_t* bits;
    const uint32_t* lambda;
    int32_t* sad;
    uint64_t* cost;
    x265amd_intra_best* best;
};

constexpr int kIntraCostWave = 64;

// lanes per job
constexpr int intra_cost_lanes(int N) { return N == 32 ? 32 : N == 16 ? 8 : 2; }

// S64: the 64x64 form (source and neighbours scaled to 32x32 while loading, no filtered buffer,
// sad << 2); N is the size the prediction runs at
template <typename P, int N, bool S64>
__global__ __launch_bounds__(kIntraCostWave) void k_intra_costs(const IntraCostArgs a)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    static_assert(!S64 || N == 32, "the 64x64 form predicts at 32x32");
    constexpr int G = intra_cost_lanes(N), JOBS = kIntraCostWave / G, SUBS = G / 2;
    constexpr int B = N == 4 ? 4 : 8;                     // sub-block edge
    constexpr int N2 = 2 * N, NS = 4 * N + 2, ND = 3 * N + 1, FS = N + 2;
    constexpr int LG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5;
    constexpr bool FILT = N >= 8 && !S64;                 // a filtered neighbour buffer exists
    constexpr bool EDGE = N <= 16;                        // DC / mode 10 / 26 edge filters (never at 32, so never S64)
    __shared__ uint16_t S[JOBS][2][NS];                   // neighbours: as loaded, filtered
    __shared__ uint16_t F[JOBS][N * FS];                  // source block
    __shared__ uint32_t D[JOBS][2][ND];                   // reference pairs of the class's current mode
    __shared__ uint32_t SAD[JOBS][36];
    __shared__ uint32_t BITS[JOBS][36];                   // mode bits (decision stage)

    const int t = threadIdx.x, slot = t / G, g = t % G;
    const int cls = g / SUBS, sub = g % SUBS;
    const int64_t job = (int64_t)xcd_block() * JOBS + slot;
    const bool live = job < a.n;
    const int64_t jj = live ? job : 0;

    // ---- load: the job's lanes read the neighbours and the source block once
    {
        const P* nb = (const P*)a.nb + a.nb_off[jj];
        constexpr int NBL = 4 * N / G;                    // neighbours per lane after scaling
        if constexpr (S64)
        {
            int v[2 * NBL];
            load_row<P, 2 * NBL>(nb + 1 + g * 2 * NBL, v);   // scale1D_128to64 on above and left alike
#pragma unroll
            for (int k = 0; k < NBL; k++) S[slot][0][1 + g * NBL + k] = (uint16_t)((v[2 * k] + v[2 * k + 1] + 1) >> 1);
        }
        else
        {
            int v[NBL];
            load_row<P, NBL>(nb + 1 + g * NBL, v);
#pragma unroll
            for (int k = 0; k < NBL; k++) S[slot][0][1 + g * NBL + k] = (uint16_t)v[k];
        }
        if (g == 0) S[slot][0][0] = (uint16_t)nb[0];

        const P* fe = (const P*)a.fenc + a.fenc_off[jj];
        if constexpr (S64)
        {
            // scale2D_64to32: lane g makes row g of the 32x32 block from source rows 2g, 2g + 1
            const P* r0 = fe + (int64_t)(2 * g) * a.fenc_stride;
            const P* r1 = r0 + a.fenc_stride;
#pragma unroll
            for (int h = 0; h < 64; h += 16)
            {
                int u[16], w[16];
                load_row<P, 16>(r0 + h, u);
                load_row<P, 16>(r1 + h, w);
#pragma unroll
                for (int k = 0; k < 8; k++)
                    F[slot][g * FS + h / 2 + k] = (uint16_t)((u[2 * k] + u[2 * k + 1] + w[2 * k] + w[2 * k + 1] + 2) >> 2);
            }
        }
        else
        {
            constexpr int RP = N / G > 0 ? N / G : 1;     // rows per lane (32: 1, 16: 2, 8: 4, 4: 2)
            constexpr int UW = N < 16 ? N : 16;
#pragma unroll
            for (int r = 0; r < RP; r++)
            {
                const int y = g * RP + r;
#pragma unroll
                for (int h = 0; h < N; h += UW)
                {
                    int u[UW];
                    load_row<P, UW>(fe + (int64_t)y * a.fenc_stride + h, u);
#pragma unroll
                    for (int k = 0; k < UW; k++) F[slot][y * FS + h + k] = (uint16_t)u[k];
                }
            }
        }
    }
    wave_sync();

    // ---- neighbour smoothing (initAdiPattern with ALL_IDX): intraFilter, or at 32x32 the strong
    // bilinear form when both threshold tests pass
    if constexpr (FILT)
    {
        const uint16_t* s = S[slot][0];
        uint16_t* f = S[slot][1];
        constexpr int NBL = 4 * N / G;
        const int tl = s[0], topLast = s[N2], leftLast = s[2 * N2];
        bool strong = false;
        if constexpr (N == 32)
        {
            const int dt = tl + topLast - 2 * (int)s[32], dl = tl + leftLast - 2 * (int)s[N2 + 32];
            strong = a.strong && abs(dt) < a.threshold && abs(dl) < a.threshold;
        }
#pragma unroll
        for (int k = 0; k < NBL; k++)
        {
            const int i = 1 + g * NBL + k;
            int o;
            if (i == N2 || i == 2 * N2) o = s[i];
            else if (strong)
            {
                const int init = (tl << 6) + N;
                o = i < N2 ? (init + (topLast - tl) * i) >> 6 : (init + (leftLast - tl) * (i - N2)) >> 6;
            }
            else
            {
                const int prev = i == N2 + 1 ? tl : (int)s[i - 1];
                o = (2 * (int)s[i] + prev + (int)s[i + 1] + 2) >> 2;
            }
            f[i] = (uint16_t)o;
        }
        if (g == 0) f[0] = (uint16_t)(strong ? tl : (2 * tl + (int)s[1] + (int)s[N2 + 1] + 2) >> 2);
        wave_sync();
    }

    // ---- the lane's sub-block of the source, in its class's frame
    int Y0 = 0, X0 = 0;
    if constexpr (N == 32)
    {
        Y0 = (((sub >> 3) & 1) * 2 + ((sub >> 1) & 1)) * 8;
        X0 = (((sub >> 2) & 1) * 2 + (sub & 1)) * 8;
    }
    else if constexpr (N == 16)
    {
        Y0 = (sub >> 1) * 8;
        X0 = (sub & 1) * 8;
    }
    constexpr bool PK = sizeof(P) == 1 && B == 8;         // packed 16-bit Hadamard (8-bit pixels)
    int fe[PK ? 1 : B][PK ? 1 : B];
    s16x2 fq[PK ? 4 : 1][PK ? 8 : 1];
    {
        const uint16_t* fj = F[slot];
        auto px = [&](int y, int x) -> int {
            return cls ? fj[(X0 + x) * FS + Y0 + y] : fj[(Y0 + y) * FS + X0 + x];
        };
        if constexpr (PK)
        {
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int x = 0; x < 8; x++) fq[k][x] = s16x2{(short)px(2 * k, x), (short)px(2 * k + 1, x)};
        }
        else
        {
#pragma unroll
            for (int y = 0; y < B; y++)
#pragma unroll
                for (int x = 0; x < B; x++) fe[y][x] = px(y, x);
        }
    }

    // ---- the class's modes: class 0 modes 18..34 then planar, class 1 modes 2..17 then DC
    const bool fh = cls != 0;
    uint32_t* Dj = D[slot][cls];
#pragma unroll 1
    for (int it = 0; it < 18; it++)
    {
        const int m = cls == 0 ? (it < 17 ? 18 + it : 0) : (it < 16 ? 2 + it : (it == 16 ? 1 : -1));
        const ModeInfo mi = decode_mode(m < 2 ? 2 : m);
        const int fsel = FILT && m >= 0 && (m == 0 || (m >= 2 && (c_intra.filter_flags[m] & N))) ? 1 : 0;
        const uint16_t* sj = S[slot][fsel];
        if (m >= 2)
        {
            // R[k], k = 0 .. 3N: R[N - 1] = top-left, above it the 2N samples of the frame's top, below it
            // the projected left samples of a negative angle (intrapred.cpp:154-164)
            const int nproj = mi.angle < 0 ? -((N * mi.angle) >> 5) - 1 : 0;
            auto Rv = [&](int k) -> uint32_t {
                if (k >= N - 1)
                {
                    const int e = k - N + 1;
                    if (e > N2) return 0;
                    return sj[flip_index(e, N2, fh)];
                }
                const int kk = N - 2 - k;
                if (kk >= nproj) return 0;
                const int i = (128 + (kk + 1) * mi.inv) >> 8;
                return sj[flip_index(N2 + i, N2, fh)];
            };
#pragma unroll
            for (int i = 0; i < 3 * N / SUBS; i++)
            {
                const int j = i * SUBS + sub;
                Dj[j] = Rv(j) | (Rv(j + 1) << 16);
            }
        }
        wave_sync();

        int v[B][B];
        if (m >= 2)
        {
#pragma unroll
            for (int y = 0; y < B; y++)
            {
                const int sum = (Y0 + y + 1) * mi.angle, f = sum & 31;
                const u16x2 wt = {(unsigned short)(32 - f), (unsigned short)f};
                const uint32_t* row = Dj + N + (sum >> 5) + X0;
#pragma unroll
                for (int x = 0; x < B; x++)
                    v[y][x] = (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, row[x]), wt, 16u, false) >> 5);
            }
            if (EDGE && mi.angle == 0 && X0 == 0)
            {
                // modes 10 / 26: first column from the frame's left neighbours (unfiltered: flags 0)
                const int r0 = (int)(Dj[N] & 0xffff), rm1 = (int)(Dj[N - 1] & 0xffff);
#pragma unroll
                for (int y = 0; y < B; y++)
                {
                    const int l = sj[flip_index(N2 + 1 + Y0 + y, N2, fh)];
                    const int e = (int16_t)(r0 + ((l - rm1) >> 1));
                    v[y][0] = e < 0 ? 0 : (e > a.maxv ? a.maxv : e);
                }
            }
        }
        else if (m == 0)
        {
            // planar, unflipped frame: above[x] = s[1 + x], left[y] = s[2N + 1 + y]
            const int trr = sj[N + 1], bl = sj[N2 + 1 + N];
            int ab[B];
#pragma unroll
            for (int x = 0; x < B; x++) ab[x] = sj[1 + X0 + x];
#pragma unroll
            for (int y = 0; y < B; y++)
            {
                const int Y = Y0 + y, lr = sj[N2 + 1 + Y];
#pragma unroll
                for (int x = 0; x < B; x++)
                {
                    const int X = X0 + x;
                    v[y][x] = ((N - 1 - X) * lr + (N - 1 - Y) * ab[x] + (X + 1) * trr + (Y + 1) * bl + N) >> (LG2 + 1);
                }
            }
        }
        else if (m == 1)
        {
            // DC in the flipped frame (its transpose): above'[x] = s[2N + 1 + x], left'[y] = s[1 + y]
            int sum = N;
            for (int i = 0; i < N; i++) sum += sj[1 + i] + sj[N2 + 1 + i];
            const int dc = sum >> (LG2 + 1);
#pragma unroll
            for (int y = 0; y < B; y++)
#pragma unroll
                for (int x = 0; x < B; x++) v[y][x] = dc;
            if (EDGE)
            {
                if (Y0 == 0)
                {
#pragma unroll
                    for (int x = 0; x < B; x++) v[0][x] = ((int)sj[N2 + 1 + X0 + x] + 3 * dc + 2) >> 2;
                }
                if (X0 == 0)
                {
#pragma unroll
                    for (int y = 0; y < B; y++) v[y][0] = ((int)sj[1 + Y0 + y] + 3 * dc + 2) >> 2;
                }
                if (Y0 == 0 && X0 == 0) v[0][0] = ((int)sj[N2 + 1] + (int)sj[1] + 2 * dc + 2) >> 2;
            }
        }
        else
        {
#pragma unroll
            for (int y = 0; y < B; y++)
#pragma unroll
                for (int x = 0; x < B; x++) v[y][x] = 0;
        }

        // Hadamard of the difference, sub-block sums joined at the reference's rounding granularity
        uint32_t r;
        if constexpr (B == 4)
        {
            int d[4][4];
#pragma unroll
            for (int y = 0; y < 4; y++)
#pragma unroll
                for (int x = 0; x < 4; x++) d[y][x] = fe[y][x] - v[y][x];
            r = had4x4_raw(d) >> 1;
        }
        else
        {
            if constexpr (PK)
            {
                s16x2 Q[4][8];
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int x = 0; x < 8; x++) Q[k][x] = fq[k][x] - s16x2{(short)v[2 * k][x], (short)v[2 * k + 1][x]};
                r = had8x8_pk(Q);
            }
            else
            {
                int d[8][8];
#pragma unroll
                for (int y = 0; y < 8; y++)
#pragma unroll
                    for (int x = 0; x < 8; x++) d[y][x] = fe[y][x] - v[y][x];
                r = had8x8(d);
            }
            if constexpr (N >= 16)
            {
                r += __shfl_xor(r, 1, 64);                 // the four 8x8 of a 16x16: one rounding
                r += __shfl_xor(r, 2, 64);
            }
            r = (r + 2) >> 2;
            if constexpr (N == 32)
            {
                r += __shfl_xor(r, 4, 64);                 // the four rounded 16x16 of a 32x32
                r += __shfl_xor(r, 8, 64);
            }
        }
        if constexpr (S64) r <<= 2;
        if (sub == 0 && m >= 0) SAD[slot][m] = r;
        wave_sync();
    }

    // ---- decision stage: sad, cost = sad + ((bits·lambda + 128) >> 8), best in the reference's order
    const uint32_t* sd = SAD[slot];
    uint32_t* bt = BITS[slot];
    const bool rd = a.mpm != nullptr;
    uint64_t lam = 0;
    if (rd)
    {
        // bits per mode: rbits, then the MPM entries last to first, so the first match wins
        const uint32_t rbits = a.bits[4 * jj + 3];
        for (int m = g; m < 35; m += G) bt[m] = rbits;
        wave_sync();
        if (g == 0)
        {
#pragma unroll
            for (int k = 2; k >= 0; k--)
            {
                const uint32_t m = a.mpm[3 * jj + k];
                if (m < 35) bt[m] = a.bits[4 * jj + k];
            }
        }
        wave_sync();
        lam = a.lambda[jj];
    }
    if (!live) return;
    auto cost_of = [&](uint32_t m) -> uint64_t {
        return rd ? (uint64_t)sd[m] + (((uint64_t)bt[m] * lam + 128) >> 8) : (uint64_t)sd[m];
    };
    for (int m = g; m < 35; m += G)
    {
        if (a.sad) a.sad[job * 35 + m] = (int32_t)sd[m];
        if (a.cost) a.cost[job * 35 + m] = cost_of(m);
    }
    if (a.best && g == 0)
    {
        uint32_t bm = 1;
        uint64_t bc = cost_of(1);
        for (uint32_t k = 1; k < 35; k++)
        {
            const uint32_t m = k == 1 ? 0 : k;             // DC, planar, 2 .. 34; strict <
            const uint64_t c = cost_of(m);
            if (c < bc) { bc = c; bm = m; }
        }
        x265amd_intra_best o;
        o.cost = bc;
        o.sad = sd[bm];
        o.bits = bt[bm];
        o.mode = bm;
        o.reserved = 0;
        a.best[job] = o;
    }
}

template <typename P, int N, bool S64>
static int launch_costs(const IntraCostArgs& a, hipStream_t st)
{
    constexpr int JOBS = kIntraCostWave / intra_cost_lanes(N);
    const dim3 grid((uint32_t)((a.n + JOBS - 1) / JOBS));
    hipLaunchKernelGGL((k_intra_costs<P, N, S64>), grid, dim3(kIntraCostWave), 0, st, a);
    return (int)hipGetLastError();
}

template <typename P>
static int launch_costs_size(int log2_size, const IntraCostArgs& a, hipStream_t st)
{
    switch (log2_size)
    {
    case 2: return launch_costs<P, 4, false>(a, st);
    case 3: return launch_costs<P, 8, false>(a, st);
    case 4: return launch_costs<P, 16, false>(a, st);
    case 5: return launch_costs<P, 32, false>(a, st);
    case 6: return launch_costs<P, 32, true>(a, st);
    }
    return X265AMD_EINVAL;
}

} // namespace x265amd

using namespace x265amd;

extern "C" int x265amd_intra_costs(int depth, int count, const x265amd_intra_cost_batch* bt, void* stream)
{
    if (depth != 8 && depth != 10 && depth != 12) return X265AMD_EINVAL;
    if (count < 0 || (count && !bt)) return X265AMD_EINVAL;
    // validate every batch before enqueuing anything
    for (int i = 0; i < count; i++)
    {
        const x265amd_intra_cost_batch& b = bt[i];
        if (b.n < 0) return X265AMD_EINVAL;
        if (!b.n) continue;                                // an empty batch is a no-op, whatever else it holds
        if (b.log2_size < 2 || b.log2_size > 6) return X265AMD_EINVAL;
        if (!b.fenc || !b.fenc_off || !b.nb || !b.nb_off) return X265AMD_EINVAL;
        if ((b.cost || b.best) && (!b.mpm || !b.bits || !b.lambda)) return X265AMD_EINVAL;
        if (!b.sad && !b.cost && !b.best) return X265AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++)
    {
        const x265amd_intra_cost_batch& b = bt[i];
        if (!b.n) continue;
        IntraCostArgs a;
        a.n = b.n;
        a.maxv = (1 << depth) - 1;
        a.strong = b.strong_smoothing;
        a.threshold = 1 << (depth - 5);
        a.fenc = b.fenc; a.fenc_stride = b.fenc_stride; a.fenc_off = b.fenc_off;
        a.nb = b.nb; a.nb_off = b.nb_off;
        // the mode bits only enter cost / best: without the three of them the kernel writes distortions only
        const bool rd = b.mpm && b.bits && b.lambda;
        a.mpm = rd ? b.mpm : nullptr; a.bits = b.bits; a.lambda = b.lambda;
        a.sad = b.sad; a.cost = b.cost; a.best = b.best;
        const int rc = depth == 8 ? launch_costs_size<uint8_t>(b.log2_size, a, st)
                                  : launch_costs_size<uint16_t>(b.log2_size, a, st);
        if (rc) return rc;
    }
    return 0;
}
