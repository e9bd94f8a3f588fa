// resnet.hip — the ResNet image tower of CLIP-ReID (custom_clip_model.ModifiedResNet,
// custom_clip_model.py:103-242; RN50 / RN101 at width 64), eval mode, the reference's GPU dtype.
//
// Activations are fp16 NHWC in HBM; convolution weights are the fp16 cast of the checkpoint's
// (utils.py:145-166 convert_weights) re-laid to [Cout][kh][kw][Cin]; BatchNorm stays out of the
// fp16 weights and is the fp32 epilogue acc * s + t (s, t from fp64 at pack time).
//
//   conv_igemm_kernel  implicit GEMM on v_mfma_f32_16x16x32_f16: M = B Ho Wo pixels, N = Cout,
//                      K = k k Cin walked as (ky, kx) ascending then channels ascending in steps
//                      of 32.  A block is 4 waves stacked along M; a wave owns 32 pixels x 16 NT
//                      output channels (NT = 4, or 2 when Cout % 64 != 0) = 2 x NT MFMA tiles.
//                      First version: every lane gathers its own fragments from global memory
//                      (16 bytes = 8 consecutive channels of one tap of one pixel, or of one
//                      weight row), no LDS stage and no barrier; an out-of-image tap is a zero
//                      fragment.  The weight fragment is the MFMA's first operand, so a lane ends
//                      up with 4 consecutive output channels of one pixel: one 8-byte NHWC store.
//   conv_stem_kernel   the 3-channel first convolution (K = 27): fp32 FMA-free chain per output
//                      channel, weights staged in LDS as fp32.
//   avgpool2_kernel    AvgPool2d(2), fp32 sum in a fixed order, one rounding.
//   attn_tokens_kernel the attention pool's rows [mean; x4] + positional_embedding (fp16) and the
//                      fp32 pooled feature; then gemm.hip (EPI_QKV, EPI_F32) and the attention
//                      kernels of attention.hip / attention_long.hip.
// Every kernel has a fixed per-element summation chain that does not depend on the batch size or
// on the pixel's position in a tile, so image b of a batch equals the same image run alone.
#include "attention.h"
#include "common.h"
#include "gemm.h"

namespace reidmi {

namespace {

constexpr int kMaxTokens = kAttnLongMax;

struct ConvArgs {
    const _Float16* x;
    const _Float16* w;
    const float* scale;
    const float* shift;
    const _Float16* resid;
    _Float16* y;
    int64_t M;  // B * Ho * Wo
    int H, W, Cin, Ho, Wo, Cout, k, stride, pad, relu;
};

// BatchNorm, residual, ReLU in fp32 (custom_clip_model.py:136-145)
__device__ __forceinline__ float bn_act(float acc, float s, float t, bool has_r, float r, int relu) {
    float v = acc * s + t;
    if (has_r) v = v + r;
    if (relu) v = fmaxf(v, 0.0f);
    return v;
}

// 4 consecutive output channels [c, c + 4) of pixel m
__device__ __forceinline__ void store4(const ConvArgs& a, int64_t m, int c, const float (&acc)[4]) {
    const float4 s = *(const float4*)(a.scale + c), t = *(const float4*)(a.shift + c);
    const int64_t o = m * a.Cout + c;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    const bool has_r = a.resid != nullptr;
    if (has_r) {
        const f16x4 rv = *(const f16x4*)(a.resid + o);
#pragma unroll
        for (int e = 0; e < 4; e++) r[e] = (float)rv[e];
    }
    f16x4 v;
    v[0] = (_Float16)bn_act(acc[0], s.x, t.x, has_r, r[0], a.relu);
    v[1] = (_Float16)bn_act(acc[1], s.y, t.y, has_r, r[1], a.relu);
    v[2] = (_Float16)bn_act(acc[2], s.z, t.z, has_r, r[2], a.relu);
    v[3] = (_Float16)bn_act(acc[3], s.w, t.w, has_r, r[3], a.relu);
    *(f16x4*)(a.y + o) = v;
}

constexpr int kConvWaveM = 32;               // pixels per wave (2 MFMA tiles)
constexpr int kConvBlockM = 4 * kConvWaveM;  // 4 waves stacked along M

template <int NT>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * kConvWaveM;
    const int n0 = blockIdx.y * (NT * 16);
    if (m0 >= a.M) return;  // whole wave (no barrier in this kernel)
    const int HoWo = a.Ho * a.Wo;
    // the two pixels whose fragments this lane gathers (MFMA operand row l15 of each M tile)
    int64_t pb[2];
    int py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int64_t m = m0 + i * 16 + l15;
        pv[i] = m < a.M;
        const int64_t mm = pv[i] ? m : 0;
        pb[i] = mm / HoWo;
        const int r = (int)(mm - pb[i] * HoWo);
        py[i] = r / a.Wo;
        px[i] = r - py[i] * a.Wo;
    }
    const int64_t Ktot = (int64_t)a.k * a.k * a.Cin;
    const _Float16* wrow[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wrow[t] = a.w + (int64_t)(n0 + t * 16 + l15) * Ktot + 8 * g;
    f32x4 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int ky = 0; ky < a.k; ky++)
        for (int kx = 0; kx < a.k; kx++) {
            const _Float16* ap[2];
            bool ok[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int iy = py[i] * a.stride + ky - a.pad, ix = px[i] * a.stride + kx - a.pad;
                ok[i] = pv[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                ap[i] = a.x + ((pb[i] * a.H + (ok[i] ? iy : 0)) * a.W + (ok[i] ? ix : 0)) * a.Cin + 8 * g;
            }
            const int64_t koff = (int64_t)(ky * a.k + kx) * a.Cin;
            for (int c0 = 0; c0 < a.Cin; c0 += 32) {
                f16x8 af[2];
#pragma unroll
                for (int i = 0; i < 2; i++) af[i] = ok[i] ? *(const f16x8*)(ap[i] + c0) : zero;
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const f16x8 bf = *(const f16x8*)(wrow[t] + koff + c0);
#pragma unroll
                    for (int i = 0; i < 2; i++)
                        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf, af[i], acc[i][t], 0, 0, 0);
                }
            }
        }
    // D[row = output channel 4 g + e][col = pixel l15] of each (i, t) tile
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int64_t m = m0 + i * 16 + l15;
        if (m >= a.M) continue;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const float v[4] = {acc[i][t][0], acc[i][t][1], acc[i][t][2], acc[i][t][3]};
            store4(a, m, n0 + t * 16 + 4 * g, v);
        }
    }
}

// Cin == 3, k == 3: one thread per (pixel, 4 output channels); weights in LDS as fp32
// sw[kk][Cout], kk = (ky * 3 + kx) * 3 + c.  Per output one chain: products (exact in fp32) added
// in kk order.
__global__ __launch_bounds__(256) void conv_stem_kernel(const ConvArgs a) {
    extern __shared__ float sw[];
    for (int e = threadIdx.x; e < 27 * a.Cout; e += blockDim.x) {
        const int n = e / 27, kk = e - n * 27;
        sw[kk * a.Cout + n] = (float)a.w[e];
    }
    __syncthreads();
    const int groups = a.Cout / 4;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = idx / groups;
    const int c = (int)(idx - m * groups) * 4;
    if (m >= a.M) return;
    const int HoWo = a.Ho * a.Wo;
    const int64_t b = m / HoWo;
    const int r = (int)(m - b * HoWo), oy = r / a.Wo, ox = r - oy * a.Wo;
    float in[27];
#pragma unroll
    for (int ky = 0; ky < 3; ky++)
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const int iy = oy * a.stride + ky - 1, ix = ox * a.stride + kx - 1;
            const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const _Float16* p = a.x + ((b * a.H + (ok ? iy : 0)) * a.W + (ok ? ix : 0)) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) in[(ky * 3 + kx) * 3 + ch] = ok ? (float)p[ch] : 0.0f;
        }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 27; kk++) {
        const float4 wv = *(const float4*)(sw + kk * a.Cout + c);
        acc[0] = acc[0] + in[kk] * wv.x;
        acc[1] = acc[1] + in[kk] * wv.y;
        acc[2] = acc[2] + in[kk] * wv.z;
        acc[3] = acc[3] + in[kk] * wv.w;
    }
    store4(a, m, c, acc);
}

int conv2d(const void* x, int64_t B, int H, int W, int Cin, const void* w, int Cout, int k, int stride,
           const float* scale, const float* shift, const void* resid, int relu, void* y, hipStream_t s) {
    RM_REQUIRE(k == 1 || k == 3, "conv2d: kernel size must be 1 or 3");
    RM_REQUIRE(stride == 1 || stride == 2, "conv2d: stride must be 1 or 2");
    RM_REQUIRE(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv2d: sizes must be positive");
    RM_REQUIRE(Cout % 32 == 0, "conv2d: Cout % 32 == 0");
    const bool stem = Cin == 3 && k == 3;
    RM_REQUIRE(stem || Cin % 32 == 0, "conv2d: Cin % 32 == 0 (or the stem's 3 channels with k = 3)");
    RM_REQUIRE(!stem || Cout <= 512, "conv2d: the 3-channel convolution takes Cout <= 512");
    const int pad = k / 2;
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const int64_t M = B * Ho * Wo;
    RM_REQUIRE(M / kConvBlockM < (1ll << 31) - 1 && B * H * W < (1ll << 40), "conv2d: too many pixels");
    if (M == 0) return OK;
    RM_REQUIRE(x && w && scale && shift && y, "conv2d: null pointer");
    ConvArgs a{(const _Float16*)x, (const _Float16*)w, scale, shift, (const _Float16*)resid, (_Float16*)y, M,
               H, W, Cin, Ho, Wo, Cout, k, stride, pad, relu};
    if (stem) {
        const int64_t threads = M * (Cout / 4);
        hipLaunchKernelGGL(conv_stem_kernel, dim3((unsigned)ceil_div(threads, 256)), dim3(256),
                           (size_t)27 * Cout * sizeof(float), s, a);
    } else if (Cout % 64 == 0) {
        hipLaunchKernelGGL(conv_igemm_kernel<4>, dim3((unsigned)ceil_div(M, kConvBlockM), Cout / 64), dim3(256), 0, s,
                           a);
    } else {
        hipLaunchKernelGGL(conv_igemm_kernel<2>, dim3((unsigned)ceil_div(M, kConvBlockM), Cout / 32), dim3(256), 0, s,
                           a);
    }
    RM_LAUNCHED();
    return OK;
}

// one thread per 8 channels of an output pixel
__global__ __launch_bounds__(256) void avgpool2_kernel(const _Float16* __restrict__ x, int64_t n8, int H, int W, int C,
                                                       _Float16* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n8) return;
    const int c8 = C / 8, Ho = H / 2, Wo = W / 2;
    const int cc = (int)(t % c8) * 8;
    int64_t p = t / c8;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const int64_t b = p / Ho;
    const _Float16* r0 = x + ((b * H + 2 * oy) * W + 2 * ox) * C + cc;
    const _Float16* r1 = r0 + (int64_t)W * C;
    const f16x8 a00 = *(const f16x8*)r0, a01 = *(const f16x8*)(r0 + C), a10 = *(const f16x8*)r1,
                a11 = *(const f16x8*)(r1 + C);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float sum = (((float)a00[e] + (float)a01[e]) + (float)a10[e]) + (float)a11[e];
        o[e] = (_Float16)(sum * 0.25f);
    }
    *(f16x8*)(y + t * 8) = o;
}

int avgpool2(const void* x, int64_t B, int H, int W, int C, void* y, hipStream_t s) {
    RM_REQUIRE(B >= 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "avgpool2: H and W must be even");
    RM_REQUIRE(C > 0 && C % 8 == 0, "avgpool2: C % 8 == 0");
    const int64_t n8 = B * (H / 2) * (W / 2) * (C / 8);
    RM_REQUIRE(n8 / 256 < (1ll << 31) - 1, "avgpool2: too many elements");
    if (n8 == 0) return OK;
    RM_REQUIRE(x && y, "avgpool2: null pointer");
    hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)ceil_div(n8, 256)), dim3(256), 0, s, (const _Float16*)x, n8, H,
                       W, C, (_Float16*)y);
    RM_LAUNCHED();
    return OK;
}

// images [B][3][H][W] (fp32 / fp16) -> fp16 NHWC [B][H][W][3], through the TTA view when tta is
// given: crop pixel (y, x) shows the flipped image at (y + top - 5, x + left - 10), the pad value
// of its channel outside (synthetic.tta_images_np with -1; the rule of encoder.hip's im2col)
struct Pad3 {
    float v[3];
};
template <typename TI>
__global__ __launch_bounds__(256) void image_view_kernel(const TI* __restrict__ img, int64_t npix, int H, int W,
                                                         const int32_t* __restrict__ tta, const Pad3 pad,
                                                         _Float16* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npix) return;
    const int x = (int)(t % W);
    const int64_t q = t / W;
    const int y = (int)(q % H);
    const int64_t b = q / H;
    int ys = y, xs = x;
    bool ok = true;
    if (tta != nullptr) {
        ys = y + tta[2 * b] - 5;
        const int xf = x + tta[2 * b + 1] - 10;
        ok = ys >= 0 && ys < H && xf >= 0 && xf < W;
        xs = W - 1 - xf;
    }
    const TI* p = img + (b * 3 * H + (ok ? ys : 0)) * W + (ok ? xs : 0);
#pragma unroll
    for (int c = 0; c < 3; c++) out[t * 3 + c] = ok ? (_Float16)p[(int64_t)c * H * W] : (_Float16)pad.v[c];
}

// AttentionPool2d's input rows (custom_clip_model.py:160-162) from x4 [B][HW][C] fp16:
// tok[b * L] = fp16(mean + pos[0]), tok[b * L + 1 + p] = fp16(x4[b][p] + pos[1 + p]), the mean
// an fp32 sum over p ascending divided by HW; pool[b] = that mean (fp32), the avg_pool2d(x4) of
// zero_shot_learning.py:89.  One thread per (image, channel).
__global__ __launch_bounds__(256) void attn_tokens_kernel(const _Float16* __restrict__ x4, int HW, int C,
                                                          const float* __restrict__ pos, _Float16* __restrict__ tok,
                                                          float* __restrict__ pool) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.x;
    if (c >= C) return;
    const _Float16* xr = x4 + b * HW * C + c;
    _Float16* tr = tok + b * (HW + 1) * C + c;
    float sum = 0.f;
    for (int p = 0; p < HW; p++) {
        const float v = (float)xr[(int64_t)p * C];
        sum = sum + v;
        tr[(int64_t)(1 + p) * C] = (_Float16)(v + pos[(int64_t)(1 + p) * C + c]);
    }
    const float mean = sum / (float)HW;
    tr[0] = (_Float16)(mean + pos[c]);
    if (pool) pool[b * C + c] = mean;
}

// fp16 NHWC [B][HW][C] -> fp32 NCHW [B][C][HW] (the reference's x3 / x4)
__global__ __launch_bounds__(256) void nhwc_to_nchw_f32_kernel(const _Float16* __restrict__ x, int64_t n, int HW, int C,
                                                               float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int p = (int)(t % HW);
    const int64_t q = t / HW;
    const int c = (int)(q % C);
    const int64_t b = q / C;
    out[t] = (float)x[(b * HW + p) * C + c];
}

// [B][L][E] -> [L][B][E] (the (HW+1)NC order AttentionPool2d returns)
__global__ __launch_bounds__(256) void lbe_kernel(const float* __restrict__ x, int64_t n, int64_t B, int L, int E,
                                                  float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int e = (int)(t % E);
    const int64_t q = t / E;
    const int64_t b = q % B, l = q / B;
    out[t] = x[(b * L + l) * E + e];
}

// ---------------------------------------------------------------- forward

int64_t al(int64_t v) { return (v + 255) & ~(int64_t)255; }

int64_t total_blocks(const int32_t (&layers)[4]) {
    return (int64_t)layers[0] + layers[1] + layers[2] + layers[3];
}

int shape_check(int width, int out_dim, int grid_h, int grid_w, const int32_t (&layers)[4], const char* who) {
    RM_REQUIRE(width > 0 && width % 64 == 0, std::string(who) + ": width % 64 == 0 (RN50 / RN101: 64)");
    RM_REQUIRE(layers[0] >= 1 && layers[1] >= 1 && layers[2] >= 1 && layers[3] >= 1 &&
                   total_blocks(layers) < (1 << 16),
               std::string(who) + ": every layer needs at least one block");
    RM_REQUIRE(out_dim > 0 && out_dim % 128 == 0, std::string(who) + ": out_dim % 128 == 0");
    RM_REQUIRE(grid_h > 0 && grid_w > 0 && (int64_t)grid_h * grid_w + 1 <= kMaxTokens,
               std::string(who) + ": the attention pool takes at most 1024 tokens (H/16 * W/16 + 1)");
    return OK;
}

int weights_check(const reidmi_resnet_weights* w) {
    RM_REQUIRE(w != nullptr && w->blocks != nullptr, "resnet: null weights");
    int rc;
    if ((rc = shape_check(w->width, w->out_dim, w->grid_h, w->grid_w, w->layers, "resnet"))) return rc;
    RM_REQUIRE(w->embed == 32 * w->width && w->heads * 64 == w->embed, "resnet: embed = 32 width = 64 heads");
    return OK;
}

int image_check(const reidmi_resnet_weights* w, int64_t B, int H, int Wimg) {
    RM_REQUIRE(B >= 0 && B < (1 << 20), "resnet: batch out of range");
    RM_REQUIRE(H > 0 && Wimg > 0 && H % 16 == 0 && Wimg % 16 == 0, "resnet: H % 16 == 0 and W % 16 == 0");
    RM_REQUIRE((int64_t)(H / 16) * (Wimg / 16) + 1 <= kMaxTokens, "resnet: too many tokens (max 1024)");
    RM_REQUIRE(H / 16 == w->grid_h && Wimg / 16 == w->grid_w,
               "resnet: image size does not match the positional-embedding grid");
    return OK;
}

struct Plan {
    int64_t img, buf[5], tok, q, k, vt, o, proj, total;
};

Plan plan(const reidmi_resnet_weights* w, int64_t B, int H, int Wimg, int full) {
    Plan p{};
    const int64_t L = (int64_t)(H / 16) * (Wimg / 16) + 1, C = w->embed;
    // the largest activation: the stem's third convolution [B][H/2][W/2][width] (= layer1's
    // [B][H/4][W/4][4 width]); every later map is smaller
    const int64_t S = B * (H / 2) * (Wimg / 2) * w->width * 2;
    int64_t off = 0;
    p.img = off; off = al(off + B * H * Wimg * 3 * 2);
    for (int i = 0; i < 5; i++) { p.buf[i] = off; off = al(off + S); }
    p.tok = off; off = al(off + B * L * C * 2);
    p.q = off; off = al(off + B * L * C * 2);
    p.k = off; off = al(off + B * L * C * 2);
    p.vt = off; off = al(off + B * C * (int64_t)attn_vt_stride((int)L) * 2);
    p.o = off; off = al(off + B * L * C * 2);
    p.proj = off; off = al(off + (full ? B * L * w->out_dim * 4 : 0));
    p.total = off;
    return p;
}

int run_conv(const reidmi_conv_weights& c, const void* x, int64_t B, int H, int W, const void* resid, int relu, void* y,
             hipStream_t s) {
    return conv2d(x, B, H, W, c.cin, c.w, c.cout, c.k, c.stride, c.scale, c.shift, resid, relu, y, s);
}

int to_nchw(const _Float16* x, int64_t B, int HW, int C, float* out, hipStream_t s) {
    const int64_t n = B * HW * C;
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, x, n, HW, C, out);
    RM_LAUNCHED();
    return OK;
}

// ---------------------------------------------------------------- packing

constexpr int64_t kAlign = 256;

struct Arena {  // offsets first (base == nullptr: sizing pass), then pointers
    char* base;
    int64_t off = 0;
    template <typename T>
    T* take(int64_t n) {
        off = (off + kAlign - 1) / kAlign * kAlign;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * (int64_t)sizeof(T);
        return p;
    }
};

// conv weight [Cout][Cin][k][k] fp32 -> [Cout][k][k][Cin] fp16
__global__ __launch_bounds__(256) void conv_relayout_kernel(const float* __restrict__ src, int64_t n, int Cin, int kk,
                                                            _Float16* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int c = (int)(t % Cin);
    const int64_t q = t / Cin;
    const int tap = (int)(q % kk);
    const int64_t o = q / kk;
    dst[t] = (_Float16)src[(o * Cin + c) * kk + tap];
}

// s = gamma / sqrt(var + eps), t = beta - mean * s in fp64, stored fp32
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ g, const float* __restrict__ b,
                                                      const float* __restrict__ mean, const float* __restrict__ var,
                                                      int n, float* __restrict__ scale, float* __restrict__ shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double sd = (double)g[i] / sqrt((double)var[i] + 1e-5);
    scale[i] = (float)sd;
    shift[i] = (float)((double)b[i] - (double)mean[i] * sd);
}

__global__ __launch_bounds__(256) void cast_f16_kernel(const float* __restrict__ src, int64_t n,
                                                       _Float16* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = (_Float16)src[t];
}

int pack_conv(Arena& a, const reidmi_convbn_src& src, int cin, int cout, int k, int stride, reidmi_conv_weights* out,
              hipStream_t s) {
    const int64_t n = (int64_t)cout * k * k * cin;
    _Float16* w = a.take<_Float16>(n);
    float* sc = a.take<float>(cout);
    float* sh = a.take<float>(cout);
    if (a.base) {
        RM_REQUIRE(src.conv_w && src.bn_w && src.bn_b && src.bn_mean && src.bn_var,
                   "resnet_weights_pack: a convolution or its BatchNorm is NULL");
        hipLaunchKernelGGL(conv_relayout_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, src.conv_w, n, cin,
                           k * k, w);
        RM_LAUNCHED();
        hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)ceil_div(cout, 256)), dim3(256), 0, s, src.bn_w, src.bn_b,
                           src.bn_mean, src.bn_var, cout, sc, sh);
        RM_LAUNCHED();
    }
    *out = reidmi_conv_weights{w, sc, sh, cin, cout, k, stride};
    return OK;
}

int pack_cast(Arena& a, const float* src, int64_t n, _Float16* dst, hipStream_t s) {
    if (a.base) {
        RM_REQUIRE(src != nullptr, "resnet_weights_pack: an attention-pool matrix is NULL");
        hipLaunchKernelGGL(cast_f16_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, src, n, dst);
        RM_LAUNCHED();
    }
    return OK;
}

int pack_copy(Arena& a, const float* src, int64_t n, float* dst, hipStream_t s) {
    if (a.base) {
        RM_REQUIRE(src != nullptr, "resnet_weights_pack: an attention-pool vector is NULL");
        RM_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return OK;
}

int resnet_pack(const reidmi_resnet_src* src, char* buf, int64_t* bytes, reidmi_resnet_weights* out,
                reidmi_bottleneck_weights* blocks, hipStream_t s) {
    RM_REQUIRE(src != nullptr && src->blocks != nullptr, "resnet_weights_pack: null source");
    int rc;
    if ((rc = shape_check(src->width, src->out_dim, src->grid_h, src->grid_w, src->layers, "resnet_weights_pack")))
        return rc;
    if (buf) RM_REQUIRE(out != nullptr && blocks != nullptr, "resnet_weights_pack: out / out_blocks required");
    Arena a{buf};
    const int w = src->width, C = 32 * w, E = src->out_dim;
    const int64_t L = (int64_t)src->grid_h * src->grid_w + 1;
    reidmi_resnet_weights tmp{};
    tmp.width = w;
    tmp.embed = C;
    tmp.heads = C / 64;
    tmp.out_dim = E;
    tmp.grid_h = src->grid_h;
    tmp.grid_w = src->grid_w;
    for (int i = 0; i < 4; i++) tmp.layers[i] = src->layers[i];
    if ((rc = pack_conv(a, src->stem[0], 3, w / 2, 3, 2, &tmp.stem[0], s)) ||
        (rc = pack_conv(a, src->stem[1], w / 2, w / 2, 3, 1, &tmp.stem[1], s)) ||
        (rc = pack_conv(a, src->stem[2], w / 2, w, 3, 1, &tmp.stem[2], s)))
        return rc;
    int inplanes = w, bi = 0;
    reidmi_bottleneck_weights dummy;
    for (int l = 0; l < 4; l++) {
        const int planes = w << l, lstride = (l == 1 || l == 2) ? 2 : 1;
        for (int i = 0; i < src->layers[l]; i++, bi++) {
            const reidmi_bottleneck_src& b = src->blocks[bi];
            reidmi_bottleneck_weights& o = blocks ? blocks[bi] : dummy;
            o = reidmi_bottleneck_weights{};
            o.stride = i == 0 ? lstride : 1;
            o.has_down = (o.stride > 1 || inplanes != planes * 4) ? 1 : 0;
            if ((rc = pack_conv(a, b.conv1, inplanes, planes, 1, 1, &o.conv1, s)) ||
                (rc = pack_conv(a, b.conv2, planes, planes, 3, 1, &o.conv2, s)) ||
                (rc = pack_conv(a, b.conv3, planes, planes * 4, 1, 1, &o.conv3, s)))
                return rc;
            if (o.has_down && (rc = pack_conv(a, b.down, inplanes, planes * 4, 1, 1, &o.down, s))) return rc;
            inplanes = planes * 4;
        }
    }
    float* pos = a.take<float>(L * C);
    _Float16* qkv = a.take<_Float16>(3 * (int64_t)C * C);
    float* qkvb = a.take<float>(3 * (int64_t)C);
    _Float16* cw = a.take<_Float16>((int64_t)E * C);
    float* cb = a.take<float>(E);
    const int64_t CC = (int64_t)C * C;
    if ((rc = pack_copy(a, src->positional_embedding, L * C, pos, s)) || (rc = pack_cast(a, src->q_w, CC, qkv, s)) ||
        (rc = pack_cast(a, src->k_w, CC, qkv + CC, s)) || (rc = pack_cast(a, src->v_w, CC, qkv + 2 * CC, s)) ||
        (rc = pack_copy(a, src->q_b, C, qkvb, s)) || (rc = pack_copy(a, src->k_b, C, qkvb + C, s)) ||
        (rc = pack_copy(a, src->v_b, C, qkvb + 2 * C, s)) || (rc = pack_cast(a, src->c_w, (int64_t)E * C, cw, s)) ||
        (rc = pack_copy(a, src->c_b, E, cb, s)))
        return rc;
    tmp.pos_emb = pos;
    tmp.qkv_w = qkv;
    tmp.qkv_b = qkvb;
    tmp.c_w = cw;
    tmp.c_b = cb;
    tmp.blocks = blocks;
    for (int c = 0; c < 3; c++) tmp.tta_pad[c] = -1.0f;
    *bytes = a.off;
    if (out) *out = tmp;
    return OK;
}

}  // namespace
}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_conv2d_f16(const void* x, int64_t B, int H, int W, int Cin, const void* w, int Cout, int k,
                                 int stride, const float* scale, const float* shift, const void* resid, int relu,
                                 void* y, void* stream) {
    return conv2d(x, B, H, W, Cin, w, Cout, k, stride, scale, shift, resid, relu, y, (hipStream_t)stream);
}

REIDMI_API int reidmi_avgpool2_f16(const void* x, int64_t B, int H, int W, int C, void* y, void* stream) {
    return avgpool2(x, B, H, W, C, y, (hipStream_t)stream);
}

REIDMI_API int64_t reidmi_resnet_pack_bytes(const reidmi_resnet_src* src) {
    int64_t n = 0;
    return resnet_pack(src, nullptr, &n, nullptr, nullptr, nullptr) ? -1 : n;
}

REIDMI_API int reidmi_resnet_weights_pack(const reidmi_resnet_src* src, void* buf, int64_t buf_bytes,
                                          reidmi_resnet_weights* out, reidmi_bottleneck_weights* out_blocks,
                                          void* stream) {
    int64_t n = 0;
    int rc;
    if ((rc = resnet_pack(src, nullptr, &n, nullptr, nullptr, nullptr))) return rc;
    RM_REQUIRE(buf != nullptr && buf_bytes >= n && ((uintptr_t)buf & (kAlign - 1)) == 0,
               "resnet_weights_pack: buffer smaller than reidmi_resnet_pack_bytes or not 256-byte aligned");
    return resnet_pack(src, (char*)buf, &n, out, out_blocks, (hipStream_t)stream);
}

REIDMI_API int64_t reidmi_resnet_workspace_bytes(const reidmi_resnet_weights* w, int64_t B, int H, int Wimg, int full) {
    if (weights_check(w) || image_check(w, B, H, Wimg)) return -1;
    return plan(w, B, H, Wimg, full).total;
}

REIDMI_API int reidmi_resnet_forward(const reidmi_resnet_weights* w, const void* images, int images_f16, int64_t B,
                                     int H, int Wimg, const int32_t* tta, int full, float* out_pool, float* out_proj,
                                     float* out_x3, float* out_x4, void* ws_, int64_t ws_bytes, void* stream) {
    int rc;
    if ((rc = weights_check(w)) || (rc = image_check(w, B, H, Wimg))) return rc;
    const Plan P = plan(w, B, H, Wimg, full);
    RM_REQUIRE(ws_bytes >= P.total, "resnet: workspace too small");
    if (B == 0) return OK;
    RM_REQUIRE(images && out_pool && out_proj && ws_, "resnet: images, out_pool, out_proj and the workspace required");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)ws_;
    _Float16* img = (_Float16*)(ws + P.img);
    _Float16 *X = (_Float16*)(ws + P.buf[0]), *Y = (_Float16*)(ws + P.buf[1]), *T1 = (_Float16*)(ws + P.buf[2]),
             *T2 = (_Float16*)(ws + P.buf[3]), *T3 = (_Float16*)(ws + P.buf[4]);
    {
        const int64_t npix = B * H * Wimg;
        const dim3 g((unsigned)ceil_div(npix, 256)), t(256);
        const Pad3 pad{{w->tta_pad[0], w->tta_pad[1], w->tta_pad[2]}};
        if (images_f16)
            hipLaunchKernelGGL(image_view_kernel<_Float16>, g, t, 0, s, (const _Float16*)images, npix, H, Wimg, tta,
                               pad, img);
        else
            hipLaunchKernelGGL(image_view_kernel<float>, g, t, 0, s, (const float*)images, npix, H, Wimg, tta, pad,
                               img);
        RM_LAUNCHED();
    }
    // the stem (custom_clip_model.py:228-232)
    int h = H / 2, wd = Wimg / 2;
    if ((rc = run_conv(w->stem[0], img, B, H, Wimg, nullptr, 1, T1, s)) ||
        (rc = run_conv(w->stem[1], T1, B, h, wd, nullptr, 1, T2, s)) ||
        (rc = run_conv(w->stem[2], T2, B, h, wd, nullptr, 1, T3, s)) ||
        (rc = avgpool2(T3, B, h, wd, w->width, X, s)))
        return rc;
    h /= 2;
    wd /= 2;
    int bi = 0;
    for (int l = 0; l < 4; l++) {
        for (int i = 0; i < w->layers[l]; i++, bi++) {
            const reidmi_bottleneck_weights& b = w->blocks[bi];
            RM_REQUIRE(b.stride == 1 || b.stride == 2, "resnet: block stride must be 1 or 2");
            if ((rc = run_conv(b.conv1, X, B, h, wd, nullptr, 1, T1, s)) ||
                (rc = run_conv(b.conv2, T1, B, h, wd, nullptr, 1, T2, s)))
                return rc;
            const _Float16* c3in = T2;
            const _Float16* idn = X;
            int ho = h, wo = wd;
            if (b.stride == 2) {
                RM_REQUIRE(b.has_down, "resnet: a strided block needs its downsample");
                ho = h / 2;
                wo = wd / 2;
                if ((rc = avgpool2(T2, B, h, wd, b.conv2.cout, T1, s)) || (rc = avgpool2(X, B, h, wd, b.conv1.cin, T2, s)) ||
                    (rc = run_conv(b.down, T2, B, ho, wo, nullptr, 0, T3, s)))
                    return rc;
                c3in = T1;
                idn = T3;
            } else if (b.has_down) {
                if ((rc = run_conv(b.down, X, B, h, wd, nullptr, 0, T3, s))) return rc;
                idn = T3;
            }
            if ((rc = run_conv(b.conv3, c3in, B, ho, wo, idn, 1, Y, s))) return rc;
            _Float16* t = X;
            X = Y;
            Y = t;
            h = ho;
            wd = wo;
        }
        if (l == 2 && full && out_x3 && (rc = to_nchw(X, B, h * wd, 16 * w->width, out_x3, s))) return rc;
    }
    RM_REQUIRE(h == w->grid_h && wd == w->grid_w, "resnet: the trunk did not end on the attention pool's grid");
    const int HW = h * wd, L = HW + 1, C = w->embed, E = w->out_dim;
    if (full && out_x4 && (rc = to_nchw(X, B, HW, C, out_x4, s))) return rc;
    // the attention pool (custom_clip_model.py:159-183)
    _Float16* tok = (_Float16*)(ws + P.tok);
    _Float16* o = (_Float16*)(ws + P.o);
    hipLaunchKernelGGL(attn_tokens_kernel, dim3((unsigned)B, (unsigned)ceil_div(C, 256)), dim3(256), 0, s, X, HW, C,
                       w->pos_emb, tok, out_pool);
    RM_LAUNCHED();
    EpiArgs ea{};
    ea.bias = w->qkv_b;
    ea.q = ws + P.q;
    ea.k = ws + P.k;
    ea.vt = ws + P.vt;
    ea.seq = L;
    ea.heads = w->heads;
    ea.lpad = attn_vt_stride(L);
    if ((rc = gemm_f16(EPI_QKV, tok, C, w->qkv_w, C, B * L, 3 * (int64_t)C, C, ea, s))) return rc;
    if ((rc = attn(ws + P.q, ws + P.k, ws + P.vt, o, B, L, w->heads, false, s))) return rc;
    EpiArgs ec{};
    ec.bias = w->c_b;
    ec.ldc = E;
    if (!full) {  // token 0 of each image only
        ec.out = out_proj;
        return gemm_f16(EPI_F32, o, (int64_t)L * C, w->c_w, C, B, E, C, ec, s);
    }
    float* proj = (float*)(ws + P.proj);
    ec.out = proj;
    if ((rc = gemm_f16(EPI_F32, o, C, w->c_w, C, B * L, E, C, ec, s))) return rc;
    const int64_t n = B * L * E;
    hipLaunchKernelGGL(lbe_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, proj, n, B, L, E, out_proj);
    RM_LAUNCHED();
    return OK;
}
