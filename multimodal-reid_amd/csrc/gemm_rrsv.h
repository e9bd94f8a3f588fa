// gemm_rrsv.h — the persistent GEMM's tile walk, and the survivor epilogue of the re-rank
// pre-filter (EPI_RRSV, gemm.h; driven by rerank_rank.hip, selection in prefilter.hip) that
// runs at the end of each of its tiles.  Device code only, compiled inside
// gemm_persistent_kernel (gemm.hip).
#pragma once
#include "gemm.h"
#include <type_traits>

namespace reidmi {

// ------------------------------------------------------------------------ gemm_walk
// A group's tile sequence t -> (M-tile, N-tile within the group): band = 0, M-major (t / tnk,
// t % tnk); band > 0, bands of `band` M-tiles walked N-major, so the tiles one XCD runs at
// once form a band x (32 / band) block and share both operands' panels in its L2 (the
// re-rank's N x N products, where neither operand fits a cache; gemm_f16).
template <bool LIST = false>
__device__ __forceinline__ void tile_mn(int t, int tnk, int band, int tiles_m, const int* list, int& mt, int& nt) {
    if constexpr (LIST) {  // EPI_RRSV's tile list (gemm.h rr_tiles)
        // constant address space: a scalar load (lgkmcnt), not a vector load whose wait would
        // drain the operand DMA in flight
        const int v = ((const __attribute__((address_space(4))) int*)list)[t];
        mt = v >> 16;
        nt = v & 0xffff;
        return;
    }
    if (band <= 0) {
        mt = t / tnk;
        nt = t - mt * tnk;
        return;
    }
    const int per = band * tnk, b = t / per, r = t - b * per;
    const int rows = tiles_m - b * band < band ? tiles_m - b * band : band;
    nt = r / rows;
    mt = b * band + (r - nt * rows);
}

#ifndef RR_GEMM_BAND
#define RR_GEMM_BAND 8
#endif

// ------------------------------------------------------------------------ survivor epilogue
// ---- EPI_RRSV (the R2 pre-filter's survivors, gemm.h) in the persistent kernel.  Per row
// group i and column group j a lane holds 4 pairs; their hi = rr_hi(acc) (packed fp32, the
// same roundings as rr_hi) is compared with the row's thresholds, and the survivors are
// appended to a per-wave buffer in LDS: 8-byte entries (tile sequence number << 13 | row in
// the wave's 128 << 6 | column in its 64, bit 31 = the pair as (column, row); hi bits), lane
// offsets from ballots.  The row and
// column records (norms, thresholds) arrive by LDS-DMA at the tile's first K-step, into one
// of two buffers by tile parity (a wave still reading tile t's records cannot be overtaken by
// tile t+2's DMA: every wave passes tile t+1's barriers in between).  So the epilogue issues
// no global memory instruction; a flush (one atomic add per entry on the row's counter, the
// pair stored at the returned position) runs when the next (i, j) group could overflow the
// buffer and once after the workgroup's last tile: typical tiles hold ~10 survivors per wave,
// so the atomic round trip is paid every few dozen tiles, not per tile.
// LDS, after the two operand stages: row records [2][256] float4 (8 KiB), column records
// [2][256] float4 (8 KiB), survivor buffers [8 waves][kRrsvWaveCap] int2 (16 KiB).
constexpr int kRrsvWaveCap = 256;  // >= one (i, j) group: 16 rows x 16 columns
constexpr int kRrsvSlotBytes = 8192 + 8192 + 8 * kRrsvWaveCap * 8;
struct RrsvWalk {
    int first, gx, wr, wc;  // the persistent walk (tile = first + seq * gx) over the tile list
    const int* list;
};

__device__ __forceinline__ void rrsv_flush(const EpiArgs& ea, uint32_t sv_lds, int& sv_n, int lane,
                                           const RrsvWalk& w) {
    for (int t0 = 0; t0 < sv_n; t0 += 64) {
        const int t = t0 + lane;
        int2 e;
        // inline ds_read: the compiler would wait for the operand DMA in flight (vmcnt(0))
        // before a plain LDS read
        asm volatile("ds_read_b64 %0, %1" : "=v"(e) : "v"(sv_lds + 8u * (uint32_t)(t < sv_n ? t : 0)) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e)::"memory");
        if (t < sv_n) {
            int mt, nt;
            tile_mn<true>(w.first + (int)(((uint32_t)e.x >> 13) & 0x3ffff) * w.gx, 1, 0, 0, w.list, mt, nt);
            const int64_t mi = (int64_t)mt * 256 + w.wr * 128 + ((e.x >> 6) & 127);
            const int ci = nt * 256 + w.wc * 64 + (e.x & 63);
            const bool tr = e.x < 0;  // bit 31: the pair belongs to the column item's row
            const int64_t m = tr ? ci : mi;
            const int col = tr ? (int)mi : ci;
            const int p = atomicAdd(ea.sv_cnt + m, 1);
            if (p < ea.sv_cap) ea.sv_list[m * ea.sv_cap + p] = make_int2(col, e.y);
        }
    }
    sv_n = 0;
}

// rows_lds / cols_lds: LDS byte addresses of this tile's record buffers (parity applied);
// both: the tile is above the diagonal of a symmetric product (rr_tri), so each pair is also
// tested as (column, row)
__device__ __forceinline__ void rrsv_tile(const EpiArgs& ea, const f32x4 (&acc)[8][4], int64_t mrow, int ncol,
                                          int64_t M, int seq, bool both, uint32_t rows_lds, uint32_t cols_lds,
                                          uint32_t sv_lds, int& sv_n, int lane, const RrsvWalk& w) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const int64_t n = ea.rr_n;
    const int cq = (lane >> 4) * 4;
    const uint64_t below = (1ull << lane) - 1;
    // appends the lane's pairs e with bit e of b: the group's total and the lanes' offsets
    // from ballots (counts 0..4), a flush first when the buffer could overflow
    auto append = [&](uint32_t b, int key, f32x4 h) {
        const uint64_t v1 = __builtin_amdgcn_ballot_w64(b != 0);
        if (v1 == 0) return;
        const int c = __builtin_popcount(b);
        const uint64_t v2 = __builtin_amdgcn_ballot_w64(c > 1), v3 = __builtin_amdgcn_ballot_w64(c > 2),
                       v4 = __builtin_amdgcn_ballot_w64(c > 3);
        const int tot = __builtin_popcountll(v1) + __builtin_popcountll(v2) + __builtin_popcountll(v3) +
                        __builtin_popcountll(v4);
        if (sv_n + tot > kRrsvWaveCap) rrsv_flush(ea, sv_lds, sv_n, lane, w);  // tot <= 256
        int p = sv_n + __builtin_popcountll(v1 & below) + __builtin_popcountll(v2 & below) +
                __builtin_popcountll(v3 & below) + __builtin_popcountll(v4 & below);
        // the whole vector reinterpreted at once: a bit_cast of one element of a float vector
        // read element 0 (hipcc 7.2)
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 hb = __builtin_bit_cast(i32x4, h);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if ((b >> e) & 1u) {
                const int2 ent = make_int2(key + e, hb[e]);
                asm volatile("ds_write_b64 %0, %1" ::"v"(sv_lds + 8u * (uint32_t)p), "v"(ent) : "memory");
                p++;
            }
        sv_n += tot;
    };
    const uint32_t ca = cols_lds + 16u * (uint32_t)(w.wc * 64 + cq);
    const uint32_t ra = rows_lds + 16u * (uint32_t)(w.wr * 128 + (lane & 15));
    // one sweep over the lane's pairs; TR: as (column, row) against the column item's
    // thresholds.  Two separate loop nests (one sweep each): a single nest with both appends
    // is too large to unroll, and the accumulators would go to scratch.
    auto sweep = [&](auto tr_c) {
        constexpr bool TR = decltype(tr_c)::value;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // columns cq + 16 j + e: (s_c, n_c, hi_max_c, lb_c)
            f32x4 cr[4];
            const uint32_t caj = ca + 256u * j;
            asm volatile("ds_read_b128 %0, %1" : "=v"(cr[0]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(cr[1]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(cr[2]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(cr[3]) : "v"(caj) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cr[0]), "+v"(cr[1]), "+v"(cr[2]), "+v"(cr[3])::"memory");
            const f2 sj0 = {cr[0][0], cr[1][0]}, sj1 = {cr[2][0], cr[3][0]};
            const f2 nj0 = {cr[0][1], cr[1][1]}, nj1 = {cr[2][1], cr[3][1]};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int64_t m = mrow + i * 16 + (lane & 15);
                f32x4 rm;  // (s_m, n_m, hi_max, lb)
                asm volatile("ds_read_b128 %0, %1" : "=v"(rm) : "v"(ra + 256u * i) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rm)::"memory");
                const f2 si = {rm[0], rm[0]}, ni = {rm[1], rm[1]};
                // hi of the pairs: rr_hi's operations on two lanes of packed fp32; as (column,
                // row) it is rr_hi with the roles swapped (the product term c_rel n_c . n_m)
                auto hi2 = [&](f2 sj, f2 nj, f2 dot) -> f2 {
                    const f2 sum = si + sj;
                    const f2 dt = __builtin_elementwise_fma(f2{-2.0f, -2.0f}, dot, sum);
                    return TR ? dt + 1.01f * (__builtin_elementwise_fma(ea.rr_c[0] * nj, ni, 0x1p-23f * sum) +
                                              ea.rr_c[1] * (nj + ni) + ea.rr_c[2])
                              : dt + 1.01f * (__builtin_elementwise_fma(ea.rr_c[0] * ni, nj, 0x1p-23f * sum) +
                                              ea.rr_c[1] * (ni + nj) + ea.rr_c[2]);
                };
                const f2 h01 = hi2(sj0, nj0, f2{acc[i][j][0], acc[i][j][1]});
                const f2 h23 = hi2(sj1, nj1, f2{acc[i][j][2], acc[i][j][3]});
                const f32x4 h = {h01.x, h01.y, h23.x, h23.y};
                // a pair survives unless lb < hi < hi_max, so a NaN or infinite bound survives
                // too and sends the row to the exact path (rank_select_sv)
                uint32_t b = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float hx = TR ? cr[e][2] : rm[2], lb = TR ? cr[e][3] : rm[3];
                    b |= (uint32_t)(m < M && ncol + j * 16 + cq + e < n && !(h[e] > hx && h[e] < lb)) << e;
                }
                const int key = (seq << 13) | ((i * 16 + (lane & 15)) << 6) | (j * 16 + cq);
                append(b, TR ? key | (int)0x80000000u : key, h);
            }
        }
    };
    sweep(std::false_type{});
    if (both) sweep(std::true_type{});
}

}  // namespace reidmi
