// encoder_calibrate.hip -- the two kernels behind the calibrated encoder open (mx_encoder_open_calibrated, encoder.hip):
//   weight_image_kernel   a Linear weight [rows, k] in f32 in HBM -> the K-blocked image [k/32][rows][32] the GEMMs read, in the
//                         four forms the host routines of encoder.hip produce (bit for bit: mx_weight_forms.h), so that the f32
//                         blob is uploaded once and every precision mode's encoder is built from it on the device
//   deviation_kernel      how far two sets of embeddings are apart, in f64 and in a fixed order
// Built with -ffp-contract=off (Makefile), like the other exact kernels.
#include "encoder_kernels.h"
#include "mx_weight_forms.h"
#include "../../include/memex_hip.h"

namespace mx {

namespace {

struct alignas(16) U16x8 {
    uint16_t v[8];
};

// One lane: eight consecutive f32 values of one row inside a 32-column block -- two 16-byte loads, one 16-byte store per
// column block of the image.  Bandwidth-bound and run once per matrix at load time: not tuned further.
__global__ __launch_bounds__(256) void weight_image_kernel(const float *__restrict__ src, size_t rows, size_t k, uint16_t *__restrict__ dst,
                                                           size_t rows_total, size_t row0, int form) {
    const size_t per_row = k >> 3;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * per_row) return;
    const size_t r = t / per_row, c = (t - r * per_row) << 3;
    const float4 lo4 = *reinterpret_cast<const float4 *>(src + r * k + c);
    const float4 hi4 = *reinterpret_cast<const float4 *>(src + r * k + c + 4);
    const uint32_t u[8] = {wf_bits(lo4.x), wf_bits(lo4.y), wf_bits(lo4.z), wf_bits(lo4.w),
                           wf_bits(hi4.x), wf_bits(hi4.y), wf_bits(hi4.z), wf_bits(hi4.w)};
    auto at = [&](size_t col) { return reinterpret_cast<U16x8 *>(dst + ((col >> 5) * rows_total + row0 + r) * 32 + (col & 31)); };
    U16x8 a, b;
    if (form == MX_PREC_BF16) {
        for (int i = 0; i < 8; ++i) a.v[i] = wf_bf16(u[i]);
        *at(c) = a;
    } else if (form == MX_PREC_BF16X3) {  // [hi | hi | lo]
        for (int i = 0; i < 8; ++i) {
            a.v[i] = wf_bf16(u[i]);
            b.v[i] = wf_bf16_lo(u[i], a.v[i]);
        }
        *at(c) = a;
        *at(k + c) = a;
        *at(2 * k + c) = b;
    } else {  // fp16: [w | w] (MX_PREC_MIXED) or [w] (MX_PREC_MIXED1)
        for (int i = 0; i < 8; ++i) a.v[i] = wf_f16_sat(u[i]);
        *at(c) = a;
        if (form == MX_PREC_MIXED) *at(k + c) = a;
    }
}

constexpr int kDevThreads = 1024, kDevWaves = kDevThreads / 64;

// the sum over a wave in a fixed tree (every lane ends with the same value)
__device__ inline double wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// sum_h x[h] y[h] in f64: lane l takes h = l, l + 64, ... in order, then the tree
__device__ inline double wave_dot(const float *x, const float *y, int H, int lane) {
    double acc = 0.0;
    for (int h = lane; h < H; h += 64) acc += (double)x[h] * (double)y[h];
    return wave_sum(acc);
}

// a, b: [B, H] f32.  out[0] = max_{i<j} |cos(a_i, a_j) - cos(b_i, b_j)|, out[1] = max_i 1 - cos(a_i, b_i); both +inf when a value
// of either set is not finite or a row has norm zero.  One workgroup: at most 2016 pairs of at most 768 terms.
__global__ __launch_bounds__(kDevThreads) void deviation_kernel(const float *__restrict__ a, const float *__restrict__ b, int B, int H,
                                                                double *__restrict__ out) {
    __shared__ double norm[2][64];
    __shared__ double wmax[2][kDevWaves];
    __shared__ int bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int t = wave; t < 2 * B; t += kDevWaves) {
        const float *x = (t < B ? a : b) + (size_t)(t < B ? t : t - B) * H;
        int nonfinite = 0;
        for (int h = lane; h < H; h += 64) nonfinite |= (wf_bits(x[h]) & 0x7f800000u) == 0x7f800000u;
        const double n = sqrt(wave_dot(x, x, H, lane));
        if (lane == 0) norm[t < B ? 0 : 1][t < B ? t : t - B] = n;
        if (nonfinite || !(n > 0.0)) bad = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    double pair = 0.0, row = 0.0;
    if (!bad) {
        const int pairs = B * (B - 1) / 2;
        for (int p = wave; p < pairs; p += kDevWaves) {
            int i = 0, q = p;
            while (q >= B - 1 - i) {
                q -= B - 1 - i;
                ++i;
            }
            const int j = i + 1 + q;
            const double ca = wave_dot(a + (size_t)i * H, a + (size_t)j * H, H, lane) / (norm[0][i] * norm[0][j]);
            const double cb = wave_dot(b + (size_t)i * H, b + (size_t)j * H, H, lane) / (norm[1][i] * norm[1][j]);
            pair = fmax(pair, fabs(ca - cb));
        }
        for (int i = wave; i < B; i += kDevWaves)
            row = fmax(row, 1.0 - wave_dot(a + (size_t)i * H, b + (size_t)i * H, H, lane) / (norm[0][i] * norm[1][i]));
    }
    if (lane == 0) {
        wmax[0][wave] = pair;
        wmax[1][wave] = row;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = 0.0, r = 0.0;
        for (int w = 0; w < kDevWaves; ++w) {
            p = fmax(p, wmax[0][w]);
            r = fmax(r, wmax[1][w]);
        }
        const double inf = __longlong_as_double(0x7ff0000000000000LL);
        out[0] = bad ? inf : p;
        out[1] = bad ? inf : r;
    }
}

}  // namespace

hipError_t launch_weight_image(hipStream_t s, const float *src, size_t rows, size_t k, uint16_t *dst, size_t rows_total, size_t row0, int form) {
    if (!src || !dst || rows < 1 || k < 32 || k % 32 || row0 + rows > rows_total || form < MX_PREC_BF16 || form > MX_PREC_MIXED1 ||
        (reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15))
        return hipErrorInvalidValue;
    const size_t items = rows * (k >> 3), blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    weight_image_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(src, rows, k, dst, rows_total, row0, form);
    return hipGetLastError();
}

hipError_t launch_embeddings_deviation(hipStream_t s, const float *a, const float *b, int B, int H, double *out2) {
    if (!a || !b || !out2 || B < 2 || B > 64 || (H != 384 && H != 768)) return hipErrorInvalidValue;
    deviation_kernel<<<dim3(1), dim3(kDevThreads), 0, s>>>(a, b, B, H, out2);
    return hipGetLastError();
}

}  // namespace mx
