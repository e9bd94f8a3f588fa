// gemm.hip — fp16 MFMA GEMM (C = A . W^T) with fused epilogues; see gemm.h.
//
// Every operand is fp16 (the reference's GPU dtype, utils.py:145-166), fp32 accumulation on
// v_mfma_f32_16x16x32_f16.  Two tilings, bit-identical per output element (same MFMA chain,
// K ascending):
//  * gemm_tile_kernel (small M: the CLS-only last block, proj, the text tower's heads):
//    128x128x64 block tile, 256 threads = 4 waves as 2x2, each wave 64x64 = 4x4 MFMA tiles;
//    operands staged global -> registers -> LDS (double-buffered, one barrier per K-step).
//  * gemm_persistent_kernel (>= 256 tiles of 256x256): see its header below.
// LDS rows are 128 B; 16-byte chunks are XOR-swizzled with (row>>1)&7 so the fragment
// reads (16 rows x 4 chunks per ds_read_b128 lane group) are bank-conflict free.  Operands
// are swapped in the MFMA (W fragment as A, activation fragment as B) so each lane ends up
// holding one output row and 4 consecutive output columns: epilogue loads/stores are 8-16 B
// per lane.
// The epilogues, the device helpers and the GEMM_VAR_* timing hooks are in gemm_epilogue.h; the
// tile walk and the re-rank pre-filter's survivor epilogue in gemm_rrsv.h; the live timing
// (reidmi_prof_*) in gemm_prof.hip; the tools-only prototype and forced-variant entry points in
// gemm_tools.hip.  Every kernel that ships is instantiated here, in this one object.
#include "gemm_epilogue.h"
#include "gemm_rrsv.h"
#include <type_traits>

namespace reidmi {

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_tile_kernel(const _Float16* __restrict__ A, int64_t lda,
                                                           const _Float16* __restrict__ W, int64_t ldw, int64_t M,
                                                           int N, int K, EpiArgs ea, int tiles_n, int nwg) {
    __shared__ __attribute__((aligned(16))) _Float16 smem[2][2][GB_M * GB_K];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
    const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    const int tm = wg / tiles_n, tn = wg % tiles_n;
    const int64_t m0 = (int64_t)tm * GB_M;
    const int n0 = tn * GB_N;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;

    // per-thread staging slots: 4 x 16 B of A and of W per K-step
    const _Float16* gA[4];
    const _Float16* gW[4];
    int soff[4];
    bool aval[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = tid + 256 * u, row = c >> 3, kc = c & 7;
        aval[u] = m0 + row < M;
        gA[u] = A + (aval[u] ? (m0 + row) : 0) * lda + kc * 8;
        gW[u] = W + (int64_t)(n0 + row) * ldw + kc * 8;
        soff[u] = swz(row, kc);
    }
    uint4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
#define GLOAD(k0)                                                                  \
    do {                                                                           \
        ra0 = aval[0] ? *(const uint4*)(gA[0] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra1 = aval[1] ? *(const uint4*)(gA[1] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra2 = aval[2] ? *(const uint4*)(gA[2] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra3 = aval[3] ? *(const uint4*)(gA[3] + (k0)) : make_uint4(0, 0, 0, 0);   \
        rw0 = *(const uint4*)(gW[0] + (k0));                                       \
        rw1 = *(const uint4*)(gW[1] + (k0));                                       \
        rw2 = *(const uint4*)(gW[2] + (k0));                                       \
        rw3 = *(const uint4*)(gW[3] + (k0));                                       \
    } while (0)
#define LSTORE(buf)                                                                \
    do {                                                                           \
        *(uint4*)(&smem[buf][0][soff[0]]) = ra0;                                   \
        *(uint4*)(&smem[buf][0][soff[1]]) = ra1;                                   \
        *(uint4*)(&smem[buf][0][soff[2]]) = ra2;                                   \
        *(uint4*)(&smem[buf][0][soff[3]]) = ra3;                                   \
        *(uint4*)(&smem[buf][1][soff[0]]) = rw0;                                   \
        *(uint4*)(&smem[buf][1][soff[1]]) = rw1;                                   \
        *(uint4*)(&smem[buf][1][soff[2]]) = rw2;                                   \
        *(uint4*)(&smem[buf][1][soff[3]]) = rw3;                                   \
    } while (0)

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    GLOAD(0);
    LSTORE(0);
    __syncthreads();
    const int nk = K / GB_K;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) GLOAD((kt + 1) * GB_K);
        const _Float16* sA = smem[cur][0];
        const _Float16* sW = smem[cur][1];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            f16x8 af[4], wf[4];
            const int kc = ks * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; i++) af[i] = *(const f16x8*)(sA + swz(wm * 64 + i * 16 + (lane & 15), kc));
#pragma unroll
            for (int j = 0; j < 4; j++) wf[j] = *(const f16x8*)(sW + swz(wn * 64 + j * 16 + (lane & 15), kc));
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = mfma16(wf[j], af[i], acc[i][j]);
        }
        if (kt + 1 < nk) LSTORE(cur ^ 1);
        __syncthreads();
    }

    // ------------------------------------------------------------------ epilogue
    if (ea.rowstat) {
        float4 bn[4];
        const int cq = (lane >> 4) * 4;
#pragma unroll
        for (int j = 0; j < 4; j++)
            bn[j] = ea.bias ? *(const float4*)(ea.bias + n0 + wn * 64 + j * 16 + cq) : make_float4(0.f, 0.f, 0.f, 0.f);
        ln_fold<4>(acc, ea.rowstat, ea.colsum, bn, m0 + wm * 64, n0 + wn * 64, M);
        epilogue_tile<EPI, 4, true>(ea, acc, m0 + wm * 64, n0 + wn * 64, M, N);
        return;
    }
    epilogue_tile<EPI, 4>(ea, acc, m0 + wm * 64, n0 + wn * 64, M, N);
#undef GLOAD
#undef LSTORE
}

// ================================================================ persistent tile
// 256x256x64 block tile, 512 threads = 8 waves as 2 (M) x 4 (N), 128x64 per wave (8x4 tiles
// of 16x16x32): half the LDS bytes per FLOP of the 64x64-per-wave 128x128 tile.  Operands go
// HBM -> LDS by global_load_lds_dwordx4 (no VGPR staging): one wave-instruction fills 1 KiB =
// 8 LDS rows of 128 B, lane l -> row 8j + l/8, physical 16-B chunk l%8.  The (row>>1)&7 XOR
// swizzle is applied on the per-lane SOURCE address (logical chunk kc = physical ^ swz(row)),
// and the same XOR on the ds_read side, so LDS stays lane-linear and fragment reads stay
// conflict-free.  All LDS is one dynamic array (a second __shared__ object makes hipcc drain
// vmcnt before every ds_read).
constexpr int G2_STAGE = (G2_M + G2_N) * GB_K;  // fp16 elements per stage

// Schedule (per K-step of 64): 4 LOAD sections (ds_read of the fragments of one 64x32
// output quadrant, issue a share of the DMA for a later K-step, lgkmcnt(0)) interleaved with
// 4 COMPUTE sections (16 register-only MFMAs), one raw s_barrier after each section.  Waves
// 4-7 run one barrier behind waves 0-3, so on every SIMD (waves w and w+4) one wave reads LDS
// while the other multiplies.  Quadrant order (0,0),(0,1),(1,1),(1,0) reuses A or W
// fragments between sections.  Region DMA: each operand stage is 4 regions of 128 LDS rows
// (16 pieces of 8 rows): A0 = rows {0..63, 128..191} (quadrant 0 of both wave rows), A1 =
// the other 128; B0 = W rows {wc*64 + 0..31}, B1 = W rows {wc*64 + 32..63}; wave w moves
// pieces 2w, 2w+1 of a region.  A region is refilled for K-step s+2 right after its last read
// in K-step s, so the only wait is one counted vmcnt(6) per K-step.
//
// Persistent: grid = min(#tiles, 256) (one workgroup per CU).  The two DMA streams — "+1"
// (region B0 of the next K-step) and "+2" (A0, B1, A1 of the K-step after) — run over the
// workgroup's concatenated (tile, K-step) sequence, so while a tile's epilogue runs, the next
// tile's first two K-steps are already landing.  Both groups run the epilogue in one barrier
// slot (their store tails overlap: +1 % c_fc, +2-6 % out_proj over running them back to
// back, profiles/r02/gemm_epilogue_sync_ab.txt).
//
// Tile walk (XCD-aware): workgroup b runs on XCD b % 8.  The XCDs are split into `ngroups`
// groups; group k owns the N-tiles [k T_n / ngroups, (k+1) T_n / ngroups), and each XCD of
// the group owns a contiguous range of that group's (M-tile, N-tile) sequence (M-major), its
// 32 workgroups striding through it — so the tiles an XCD runs at once share A row panels in
// its L2, and with ngroups > 1 the W panels an XCD re-reads shrink to its N share.
//
// Deferred epilogue stores: the epilogue's stores are not waited for by the next tile's first
// K-step.  vmcnt retires in issue order, so a plain `vmcnt(6)` after an epilogue would wait
// for every store the epilogue issued (one HBM write round trip per tile, MFMAs idle).  The
// next tile's first "+1" DMA (B0 of its K-step 1) is issued BEFORE the epilogue, and that
// step's wait counts the epilogue's memory instructions as allowed to be outstanding:
// vmcnt(6 + S (+ the tile's bias / colsum / rowstat DMAs)), S = EpiVm<EPI>::count (global
// load/store instructions per wave and full tile, counted from the ISA; with LayerNorm
// partials the residual epilogue issues 8 more stores, so S is then a lower bound — safe,
// as vmcnt retires in order).  Only after a full tile (no masked rows) and not for
// scattered-v^T QKV tiles; otherwise the plain vmcnt(6).  The bias is read from LDS by
// inline ds_read (the compiler would insert a vmcnt(0) before a ds_read of an LDS-DMA'd
// slot, draining the in-flight DMA every tile).  All tilings run the same MFMA chain per
// output element -> bit-identical results.
// TAG: a symbol tag only (same code): the residual epilogue's two callers, out_proj (K = W,
// TAG 0) and mlp.c_proj (K = 4W, TAG 1), get their own kernel names in rocprof traces
template <int EPI, int TAG = 0>
__global__ __launch_bounds__(512, 2) void gemm_persistent_kernel(const _Float16* __restrict__ A, int64_t lda,
                                                                 const _Float16* __restrict__ W, int64_t ldw,
                                                                 int64_t M, int N, int K, EpiArgs ea, int tiles_m,
                                                                 int tiles_n, int ngroups, int band) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int G = gridDim.x;
    const int bid = blockIdx.x;
    const int ng = G < 8 ? G : 8;
    const int xg = bid % ng, gx = G / ng + ((G % ng) > xg ? 1 : 0);
    const int ngr = (ng == 8 && 8 % ngroups == 0 && ngroups <= tiles_n) ? ngroups : 1;
    const int xper = ng / ngr, grp = xg / xper, xs = xg - grp * xper;
    const int nb0 = tiles_n * grp / ngr, tnk = tiles_n * (grp + 1) / ngr - nb0;  // this group's N-tiles
    const int64_t sub = (int64_t)tiles_m * tnk;
    const int lo = (int)(sub * xs / xper), hi = (int)(sub * (xs + 1) / xper);
    const int first = lo + bid / ng;
    if (first >= hi) return;
    if constexpr (EPI == EPI_RESID_F16) {
        // The residual epilogue reads and writes 2 x 128 KB per tile; with every workgroup in
        // step those bursts hit HBM together.  Odd workgroups start ~8k cycles (~1/8 of an
        // out_proj tile) late: out_proj -2.5 %, c_proj -1.7 %; no effect on the other epilogues
        // (profiles/r04/gemm_stagger_prefetch_ab.txt)
        if (bid & 1) __builtin_amdgcn_s_sleep(127);
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    const int nk = K / GB_K;

    // per-lane DMA geometry: piece pc = 2*wid + u of region half h
    int rowA[2][2], kcA[2][2], offA[2][2], offW[2][2];
    uint32_t offAb[2][2], offWb[2][2];  // byte offsets from the tile's (row 0, k0) element
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int pc = 2 * wid + u;
            const int ra = 128 * (pc >> 3) + 64 * h + 8 * (pc & 7);
            const int rb = 64 * (pc >> 2) + 32 * h + 8 * (pc & 3);
            const int r1 = ra + (lane >> 3), r2 = rb + (lane >> 3);
            rowA[h][u] = r1;
            kcA[h][u] = ((lane & 7) ^ ((r1 >> 1) & 7)) * 8;
            offAb[h][u] = (uint32_t)(r1 * (int)lda + kcA[h][u]) * 2u;
            offWb[h][u] = (uint32_t)(r2 * (int)ldw + ((lane & 7) ^ ((r2 >> 1) & 7)) * 8) * 2u;
            offA[h][u] = ra * GB_K;
            offW[h][u] = G2_M * GB_K + rb * GB_K;
        }
    const int* const rr_list = EPI == EPI_RRSV ? ea.rr_tiles : nullptr;  // (gemm.h rr_tiles)
    if constexpr (EPI != EPI_RRHI) band = 0;  // bands: the re-rank's dense product only
    // a DMA stream position: tile (m0, n0), K-step, and whether all 256 A rows exist
    // a: byte address of A[m0][kt * GB_K], w: of W[n0][kt * GB_K] -- computed once per tile
    // and stepped by one K-step's bytes, so a DMA issue costs no 64-bit multiply (scalar
    // instructions of the LOAD phases, which run beside the partner wave's MFMAs)
    struct Pos {
        int tile, kt;
        int64_t m0;
        int n0;
        bool full;
        const char* a;
        const char* w;
    };
    auto set_tile = [&](Pos& p, int tile) {
        p.tile = tile;
        p.kt = 0;
        int mt, nt;
        tile_mn<EPI == EPI_RRSV>(tile, tnk, band, tiles_m, rr_list, mt, nt);
        p.m0 = (int64_t)mt * G2_M;
        p.n0 = (nb0 + nt) * G2_N;
        p.full = p.m0 + G2_M <= M;
        p.a = (const char*)(A + (GEMM_VAR_ASAME ? 0 : p.m0) * lda);
        p.w = (const char*)(W + (int64_t)p.n0 * ldw);
    };
    auto advance = [&](Pos& p) {
        if (++p.kt == nk) {
            set_tile(p, p.tile + gx);
        } else {
            p.a += GB_K * 2;
            p.w += GB_K * 2;
        }
    };
    // uniform tile base + per-lane 32-bit byte offset (SGPR base + VGPR offset form)
    auto issue_a = [&](int stage, int h, const Pos& p) {
        const char* base = p.a;
        if (p.full) {
#pragma unroll
            for (int u = 0; u < 2; u++)
                __builtin_amdgcn_global_load_lds(base + offAb[h][u],
                                                 (lds_ptr_t)(lds + stage * G2_STAGE + offA[h][u]), 16, 0, 0);
        } else {  // partial last row tile: rows >= M read row M-1 (never stored)
            const int lim = (int)(M - p.m0);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int r = rowA[h][u] < lim ? rowA[h][u] : lim - 1;
                __builtin_amdgcn_global_load_lds(base + (uint32_t)(r * (int)lda + kcA[h][u]) * 2u,
                                                 (lds_ptr_t)(lds + stage * G2_STAGE + offA[h][u]), 16, 0, 0);
            }
        }
    };
    auto issue_w = [&](int stage, int h, const Pos& p) {
        const char* base = p.w;
#pragma unroll
        for (int u = 0; u < 2; u++)
            __builtin_amdgcn_global_load_lds(base + offWb[h][u],
                                             (lds_ptr_t)(lds + stage * G2_STAGE + offW[h][u]), 16, 0, 0);
    };
#define G5_BARRIER()                              \
    do {                                          \
        __builtin_amdgcn_sched_barrier(0);        \
        __builtin_amdgcn_s_barrier();             \
        __builtin_amdgcn_sched_barrier(0);        \
    } while (0)
#define G5_LDS_DONE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

    // Both column halves' W fragments stay in registers (6 more VGPRs as allocated), so
    // LOAD 3 reads nothing: the K-step's W fragments are read from LDS once, not 1.5 times
    // (-14 % LDS read bytes; c_fc / QKV / c_proj +1 %, out_proj even,
    // profiles/r04/gemm_fb2_ab.txt)
    f16x8 fa[4][2], fbq[2][2][2];
    f32x4 acc[8][4];
    auto load_a = [&](const _Float16* sA, int qm) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                fa[i][ks] = *(const f16x8*)(sA + swz(wr * 128 + qm * 64 + i * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    auto load_b = [&](const _Float16* sW, int qn) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                fbq[qn][j][ks] =
                    *(const f16x8*)(sW + swz(wc * 64 + qn * 32 + j * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    // FIRST: the tile's first K-step starts every accumulator chain from an inline-constant 0
    // C operand, so no zeroing moves run between tiles (64 v_mov_b64 per wave and tile)
    auto compute = [&](int qm, int qn, auto firstc) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    f32x4& c = acc[qm * 4 + i][qn * 2 + j];
                    const f16x8& b = fbq[qn][j][ks];
                    if constexpr (decltype(firstc)::value)
                        c = mfma16(b, fa[i][ks], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : c);
                    else
                        c = mfma16(b, fa[i][ks], c);
                }
    };

    // Bias of the current tile: one LDS-DMA per wave at the tile's first K-step into the
    // wave's own 1 KB slot (lane l -> bias[n0 + 4l .. 4l+3]); issued before that step's
    // B0 DMA, so the step's vmcnt(6) retires it.  The epilogue reads it with ds_read.
    const bool has_bias = EPI != EPI_PATCH && ea.bias != nullptr;
    float* bias_slot = (float*)(lds + 2 * G2_STAGE) + wid * 256;
    // Folded LayerNorm: colsum of the tile's 256 columns and (rstd, -mean rstd) of the
    // wave's 128 rows go to LDS by the same DMA at the tile's first K-step (the rowstat
    // buffer is padded to whole 256-row tiles, gemm.h).
    const bool fold = EPI != EPI_RESID_F16 && ea.rowstat != nullptr;  // (gemm_f16 rejects a residual fold)
    float* cs_slot = bias_slot + 8 * 256;
    float* rs_slot = bias_slot + 16 * 256;
    // streams: p1 = step s+1 (region B0), p2 = step s+2 (A0, B1, A1); requires nk >= 2
    Pos p1, p2;
    {
        Pos p0;
        set_tile(p0, first);
        issue_a(0, 0, p0);
        issue_a(0, 1, p0);
        issue_w(0, 0, p0);
        issue_w(0, 1, p0);
        p1 = p0;
        advance(p1);  // step 1: always inside the first tile (nk >= 2)
        issue_a(1, 0, p1);
        issue_w(1, 1, p1);
        issue_a(1, 1, p1);
        p2 = p1;
        advance(p2);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    __syncthreads();
    if (wr == 1) G5_BARRIER();
    // EPI_RRSV (rrsv_tile): record buffers and the wave's survivor buffer after the stages
    char* const rr_slot = (char*)(lds + 2 * G2_STAGE);
    const uint32_t rr_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)rr_slot;
    const uint32_t sv_lds = rr_lds + 8192 + 8192 + 8u * kRrsvWaveCap * (uint32_t)wid;
    int sv_n = 0;  // wave-uniform
    int seq = 0;   // tiles done by this workgroup
    int buf = 0;
    constexpr bool CAN_DEFER = EpiVm<EPI>::count > 0;
    bool deferred = false;  // the previous tile's epilogue stores may still be in flight
    for (int tile = first; tile < hi; tile += gx) {
        int tmt, tnt;  // this tile's M-tile and N-tile (within the group)
        tile_mn<EPI == EPI_RRSV>(tile, tnk, band, tiles_m, rr_list, tmt, tnt);
        auto kstep = [&](int kt, auto firstc) {
            const bool has1 = p1.tile < hi, has2 = p2.tile < hi;
            const bool b0_early = CAN_DEFER && kt == 0 && tile != first;  // issued before the epilogue
            const _Float16* sA = lds + buf * G2_STAGE;
            const _Float16* sW = sA + G2_M * GB_K;
            // LOAD 0 / COMPUTE (0,0)
            load_a(sA, 0);
            load_b(sW, 0);
            if (kt == 0 && has_bias)
                __builtin_amdgcn_global_load_lds(ea.bias + (nb0 + tnt) * G2_N + lane * 4, (lds_ptr_t)bias_slot,
                                                 16, 0, 0);
            if (kt == 0 && fold) {
                __builtin_amdgcn_global_load_lds(ea.colsum + (nb0 + tnt) * G2_N + lane * 4, (lds_ptr_t)cs_slot,
                                                 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const float*)(ea.rowstat + (int64_t)tmt * G2_M + wr * 128) +
                                                     lane * 4,
                                                 (lds_ptr_t)rs_slot, 16, 0, 0);
            }
            if constexpr (EPI == EPI_RRSV) {
                // this tile's row / column records (rrsv_tile), one 1 KiB piece per wave
                if (kt == 0) {
                    const int par = seq & 1;
                    if (wid < 4)
                        __builtin_amdgcn_global_load_lds(ea.rr_rowmeta + (int64_t)tmt * G2_M + wid * 64 + lane,
                                                         (lds_ptr_t)(rr_slot + par * 4096 + wid * 1024), 16, 0, 0);
                    else
                        __builtin_amdgcn_global_load_lds(ea.rr_colrec + (int64_t)(nb0 + tnt) * G2_N + (wid - 4) * 64 + lane,
                                                         (lds_ptr_t)(rr_slot + 8192 + par * 4096 + (wid - 4) * 1024),
                                                         16, 0, 0);
                }
            }
            constexpr bool KDMA = GEMM_VAR_NODMA == 0;
            if (KDMA && has1 && !b0_early) issue_w(buf ^ 1, 0, p1);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(0, 0, firstc);
            G5_BARRIER();
            // LOAD 1 / COMPUTE (0,1)
            load_b(sW, 1);
            if (KDMA && has2) issue_a(buf, 0, p2);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(0, 1, firstc);
            G5_BARRIER();
            // LOAD 2 / COMPUTE (1,1)
            load_a(sA, 1);
            if (KDMA && has2) issue_w(buf, 1, p2);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(1, 1, firstc);
            G5_BARRIER();
            // LOAD 3 (no LDS reads: W fragments of column half 0 are still in fbq[0]) / COMPUTE (1,0)
            if (has2) {
                if constexpr (KDMA) issue_a(buf, 1, p2);
                G5_LDS_DONE();
                if constexpr (CAN_DEFER) {
                    constexpr int S = EpiVm<EPI>::count;
                    if (kt == 0 && deferred) {  // + the first K-step's bias / colsum / rowstat DMAs
                        if (fold)
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 9) : "memory");
                        else if (has_bias)
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 7) : "memory");
                        else
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 6) : "memory");
                    } else if constexpr (!GEMM_VAR_NOWAIT) {
                        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    }
                } else if constexpr (!GEMM_VAR_NOWAIT) {
                    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                }
            } else {
                G5_LDS_DONE();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            G5_BARRIER();
            compute(1, 0, firstc);
            G5_BARRIER();
            advance(p1);
            advance(p2);
            buf ^= 1;
        };
        kstep(0, std::true_type{});  // nk >= 2 (launch: K >= 2 * GB_K)
        for (int kt = 1; kt < nk; ++kt) kstep(kt, std::false_type{});
        // both wave groups run the epilogue in the same barrier slot (group A, one barrier ahead
        // in the K-loop, waits here for group B's last COMPUTE; B catches up after it), so the
        // two groups' store tails overlap instead of running back to back
        if (wr == 0) G5_BARRIER();
        const int64_t m0 = (int64_t)tmt * G2_M;
        const int n0 = (nb0 + tnt) * G2_N;
        if constexpr (CAN_DEFER) {
            deferred = false;
            if (p1.tile < hi) {  // a next tile exists: issue its K-step 1 B0 (skipped in its LOAD 0)
                issue_w(buf ^ 1, 0, p1);
                deferred = m0 + G2_M <= M;
                if constexpr (EPI == EPI_QKV) deferred = deferred && (n0 + ea.n_off) / (ea.heads * 64) != 2;
                // the distance form's masked / unaligned stores vary in number: not deferred
                if constexpr (EPI == EPI_F32) deferred = deferred && ea.dist_rsq == nullptr;
            }
        }
        // residual epilogue: its row reads go out before the bias arithmetic (after the next
        // tile's early DMA, so the deferred-store count EpiVm is unchanged), their latency
        // then runs beside it
        constexpr bool RPRE = EPI == EPI_RESID_F16 && !GEMM_VAR_NORESLOAD;
        f16x8 xres[RPRE ? 8 : 1][2];
        if constexpr (RPRE) resid_rows_load<8>(ea, m0 + wr * 128, n0 + wc * 64, M, xres);
        if (has_bias) {
            f32x4 b[4];
            // inline ds_read: no compiler-inserted vmcnt(0) for the LDS-DMA'd slot (retired by
            // the tile's first K-step wait)
            const float* bp = bias_slot + wc * 64 + (lane >> 4) * 4;
            const uint32_t ba = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)bp;
            asm volatile("ds_read_b128 %0, %1" : "=v"(b[0]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(b[1]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(b[2]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(b[3]) : "v"(ba) : "memory");
            // the wait names the read registers: no use of them can be scheduled above it (the
            // hardware does not track VGPRs written by an outstanding LDS read)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])::"memory");
            // acc <- rstd * acc + (-mean rstd * s_n + b'_n); without a fold (rstd, s) = (1, 0):
            // fma(1, acc, fma(0, 0, b)) == acc + b exactly.  One branch-free update (a branch on
            // acc would duplicate the 128 accumulators).
            f32x4 sn[4];
            f32x2v rs[8];
            if (fold) {
                const uint32_t ca = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(
                    cs_slot + wc * 64 + (lane >> 4) * 4);
                const uint32_t ra =
                    (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(rs_slot + (lane & 15) * 2);
                asm volatile("ds_read_b128 %0, %1" : "=v"(sn[0]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(sn[1]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(sn[2]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(sn[3]) : "v"(ca) : "memory");
                asm volatile("ds_read_b64 %0, %1" : "=v"(rs[0]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:128" : "=v"(rs[1]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:256" : "=v"(rs[2]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:384" : "=v"(rs[3]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:512" : "=v"(rs[4]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:640" : "=v"(rs[5]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:768" : "=v"(rs[6]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:896" : "=v"(rs[7]) : "v"(ra) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(sn[0]), "+v"(sn[1]), "+v"(sn[2]), "+v"(sn[3]), "+v"(rs[0]), "+v"(rs[1]), "+v"(rs[2]),
                               "+v"(rs[3]), "+v"(rs[4]), "+v"(rs[5]), "+v"(rs[6]), "+v"(rs[7])::"memory");
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) sn[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 8; i++) rs[i] = f32x2v{1.f, 0.f};
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i][j][0] = __builtin_fmaf(rs[i].x, acc[i][j][0], __builtin_fmaf(rs[i].y, sn[j].x, b[j].x));
                    acc[i][j][1] = __builtin_fmaf(rs[i].x, acc[i][j][1], __builtin_fmaf(rs[i].y, sn[j].y, b[j].y));
                    acc[i][j][2] = __builtin_fmaf(rs[i].x, acc[i][j][2], __builtin_fmaf(rs[i].y, sn[j].z, b[j].z));
                    acc[i][j][3] = __builtin_fmaf(rs[i].x, acc[i][j][3], __builtin_fmaf(rs[i].y, sn[j].w, b[j].w));
                }
        }
        if constexpr (EPI == EPI_RRSV)
            rrsv_tile(ea, acc, m0 + wr * 128, n0 + wc * 64, M, seq, ea.rr_tri && tmt < tnt, rr_lds + (seq & 1) * 4096,
                      rr_lds + 8192 + (seq & 1) * 4096, sv_lds, sv_n, lane,
                      RrsvWalk{first, gx, wr, wc, rr_list});
        else if (EPI == EPI_GELU_H16 && m0 + G2_M <= M)  // c_fc's full tiles: no row checks
            epilogue_tile<EPI, 8, true, RPRE, true>(ea, acc, m0 + wr * 128, n0 + wc * 64, M, N, xres);
        else
            epilogue_tile<EPI, 8, true, RPRE>(ea, acc, m0 + wr * 128, n0 + wc * 64, M, N, xres);
        seq++;
        if (wr == 1) G5_BARRIER();
    }
    if constexpr (EPI == EPI_RRSV)
        rrsv_flush(ea, sv_lds, sv_n, lane, RrsvWalk{first, gx, wr, wc, rr_list});
    if (wr == 0) G5_BARRIER();
#undef G5_BARRIER
#undef G5_LDS_DONE
}

template <int EPI>
static int launch(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                  const EpiArgs& ea, hipStream_t s, const GemmOpts& opt) {
    const bool listed = EPI == EPI_RRSV;  // walks a tile list (gemm.h rr_tiles)
    RM_REQUIRE(!listed || (ea.rr_tiles && ea.rr_ntiles > 0), "gemm: the survivor epilogue needs its tile list");
    const int64_t tiles256 = listed ? ea.rr_ntiles : (int64_t)ceil_div(M, G2_M) * (N / G2_N);
    const bool fits = N % G2_N == 0 && K >= 2 * GB_K && lda * G2_M < (1ll << 31) && ldw * G2_N < (1ll << 31);
    if (fits && (opt.tile == 2 || (opt.tile == 0 && tiles256 >= 256))) {
        // a tile list is walked as tiles_m = its length x 1 N-tile, one XCD group
        const int tiles_m = listed ? (int)tiles256 : ceil_div(M, G2_M), tiles_n = listed ? 1 : (int)(N / G2_N);
        RM_REQUIRE(tiles256 < (1ll << 31), "gemm: grid too large");
        RM_REQUIRE(!listed || (ceil_div(M, G2_M) <= 65536 && N / G2_N <= 65536), "gemm: tile list: too many tiles");
        RM_REQUIRE(EPI != EPI_RRSV || tiles256 / (tiles256 < 256 ? tiles256 : 256) < (1 << 18),
                   "gemm: survivor epilogue: too many tiles per workgroup");
        // two operand stages + bias / colsum / rowstat slots (8 waves x 1 KiB each)
        // (EPI_RRSV: its record and survivor buffers instead, rrsv_tile)
        const size_t lds = 2 * (size_t)G2_STAGE * 2 + (EPI == EPI_RRSV ? kRrsvSlotBytes : 3 * 8 * 256 * sizeof(float));
        // c_proj (residual epilogue, K > N) launches the TAG 1 copy of the kernel
        const bool tag1 = EPI == EPI_RESID_F16 && K > N;
        auto kern = tag1 ? gemm_persistent_kernel<EPI, EPI == EPI_RESID_F16 ? 1 : 0> : gemm_persistent_kernel<EPI, 0>;
        static bool attr[2] = {false, false};
        if (!attr[tag1]) {
            RM_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr[tag1] = true;
        }
        const int grid = (int)(tiles256 < 256 ? tiles256 : 256);
        // XCD N-groups: auto = 2 when the N-tiles split evenly and there are >= 8 of them
        // (c_fc: 12 tiles, +2 %, 15 % less L2 fetch; an uneven split idles the XCDs of the
        // smaller group), else 1 (profiles/r02/walk_ab.txt)
        const int ngroups =
            listed ? 1 : opt.ngroups > 0 ? opt.ngroups : (tiles_n % 2 == 0 && tiles_n >= 8 ? 2 : 1);
        // bands of M-tiles: auto = 8 for the re-rank's dense N x N product (both operands
        // stream from HBM; the survivor epilogue's tile list is in band order too), else
        // M-major (the encoder's weights stay in L2 / MALL)
        const int band = EPI != EPI_RRHI ? 0 : opt.band >= 0 ? opt.band : RR_GEMM_BAND;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, s, (const _Float16*)A,
                           lda, (const _Float16*)W, ldw, M, (int)N, (int)K, ea, tiles_m, tiles_n, ngroups, band);
        RM_LAUNCHED();
        return OK;
    }
    if constexpr (EPI == EPI_RRSV) {
        return fail(EINVAL_, "gemm: the survivor epilogue runs on the persistent 256 x 256 tile only "
                             "(N % 256 == 0, K >= 128, >= 256 tiles)");
    } else {
    const int tiles_m = ceil_div(M, GB_M), tiles_n = (int)(N / GB_N);
    const int64_t nwg = (int64_t)tiles_m * tiles_n;
    RM_REQUIRE(nwg < (1ll << 31), "gemm: grid too large");
    hipLaunchKernelGGL((gemm_tile_kernel<EPI>), dim3((unsigned)nwg), dim3(256), 0, s, (const _Float16*)A, lda,
                       (const _Float16*)W, ldw, M, (int)N, (int)K, ea, tiles_n, (int)nwg);
    RM_LAUNCHED();
    return OK;
    }
}

int gemm_f16(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
             const EpiArgs& ea, hipStream_t s, const GemmOpts& opt) {
    RM_REQUIRE(opt.tile >= 0 && opt.tile <= 2, "gemm tile: 0 auto, 1 128x128, 2 persistent 256x256");
    RM_REQUIRE(opt.band >= -1 && opt.band <= 64, "gemm walk: band in -1 (auto) .. 64");
    RM_REQUIRE(opt.ngroups == 0 || opt.ngroups == 1 || opt.ngroups == 2 || opt.ngroups == 4 || opt.ngroups == 8,
               "gemm walk: ngroups in {0 (auto), 1, 2, 4, 8}");
    RM_REQUIRE(M >= 0 && N > 0 && K > 0, "gemm: bad shape");
    RM_REQUIRE((epi != EPI_QKV && epi != EPI_PATCH) || M < (1ll << 31), "gemm: head split / patch rows need M < 2^31");
    RM_REQUIRE(N % GB_N == 0 && K % GB_K == 0, "gemm: needs N % 128 == 0 and K % 64 == 0");
    RM_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "gemm: lda/ldw must be >= K and 16-byte rows");
    RM_REQUIRE((epi != EPI_H16 && epi != EPI_GELU_H16 && epi != EPI_RESID_F16) ||
                   (ea.ldc % 8 == 0 && ((uintptr_t)ea.out & 15) == 0 && ea.ldc < (1 << 24) && N < (1 << 24)),
               "gemm: fp16 output needs ldc % 8 == 0 (< 2^24) and a 16-byte aligned base");
    RM_REQUIRE((ea.rowstat == nullptr) == (ea.colsum == nullptr), "gemm: rowstat and colsum go together");
    RM_REQUIRE(ea.rowstat == nullptr || ea.bias != nullptr, "gemm: a folded LayerNorm needs the folded bias");
    RM_REQUIRE(epi != EPI_RESID_F16 || ea.rowstat == nullptr, "gemm: the residual epilogue takes no folded LayerNorm");
    RM_REQUIRE(ea.dist_rsq == nullptr || (epi == EPI_F32 && ea.dist_csq != nullptr && ea.dist_n > 0 &&
                                          ea.dist_n <= N && ea.ldc >= ea.dist_n && ea.bias == nullptr),
               "gemm: the distance form needs EPI_F32, both norm vectors, 0 < dist_n <= N, ldc >= dist_n, no bias");
    if (M == 0) return OK;
    hipEvent_t ev_b = nullptr;  // live timing (gemm_prof.hip): stays null while it is off
    if (const int prc = prof_begin(2.0 * (double)M * (double)N * (double)K, epi, s, &ev_b)) return prc;
    int rc;
    switch (epi) {
        case EPI_H16: rc = launch<EPI_H16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_GELU_H16: rc = launch<EPI_GELU_H16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_QKV: rc = launch<EPI_QKV>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_PATCH: rc = launch<EPI_PATCH>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_F32: rc = launch<EPI_F32>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RESID_F16: rc = launch<EPI_RESID_F16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RRHI: rc = launch<EPI_RRHI>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RRSV: rc = launch<EPI_RRSV>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        default: return fail(EINVAL_, "gemm: unknown epilogue");
    }
    if (ev_b)
        if (const int prc = prof_end(ev_b, s)) return prc;
    return rc;
}

int gemm_api(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
             const float* bias, const void* rowstat, const float* colsum, void* out, int64_t ldc, const GemmOpts& opt,
             void* stream) {
    RM_REQUIRE(epi == EPI_H16 || epi == EPI_GELU_H16 || epi == EPI_F32 || epi == EPI_RESID_F16,
               "reidmi_gemm_f16: epi must be 0 (fp16), 1 (QuickGELU fp16), 5 (fp32) or 6 (fp16 residual)");
    EpiArgs ea{};
    ea.out = out;
    ea.ldc = ldc;
    ea.bias = bias;
    ea.rowstat = (const float2*)rowstat;
    ea.colsum = colsum;
    return gemm_f16(epi, A, lda, W, ldw, M, N, K, ea, (hipStream_t)stream, opt);
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_gemm_f16(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N,
                               int64_t K, const float* bias, const void* rowstat, const float* colsum, void* out,
                               int64_t ldc, void* stream) {
    return gemm_api(epi, A, lda, W, ldw, M, N, K, bias, rowstat, colsum, out, ldc, GemmOpts{}, stream);
}
