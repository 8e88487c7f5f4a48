// ims_readout.h -- section of the one translation unit (imsim_hip.hip): CCD readout -- bleed trails, amplifier segments, CTE,
// noise and digitisation.
//
// Kernels: k_readout_span_init, k_readout_flags, k_readout_bleed, k_readout_segments, k_readout_cte, k_readout_finish_pairs,
// k_readout_finish.
// Entry points: ims_readout_bleed, ims_readout_segments, ims_readout_cte, ims_readout_finish.
#pragma once

// ---------------- CCD readout (imsim/readout.py:413-478, imsim/bleed_trails.py) ----------------
constexpr long long READOUT_ID_BASE = 0x7E00000000ll;   // object id space of the read-noise streams (+ amp index)

// span[4 x + 2 half + {0,1}]: first / last saturated row of the channel (relative to the channel's first row)
__global__ __launch_bounds__(256) void k_readout_span_init(int* __restrict__ span, int nx)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nx) { span[4 * x] = 0x7FFFFFFF; span[4 * x + 1] = -1; span[4 * x + 2] = 0x7FFFFFFF; span[4 * x + 3] = -1; }
}

__global__ __launch_bounds__(256) void k_readout_flags(const double* __restrict__ image, unsigned char* __restrict__ flags,
                                                       int* __restrict__ span, int nx, int ny, double full_well, int midline_stop)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)nx * ny) return;
    const bool sat = image[p] > full_well;
    flags[p] = sat ? 1 : 0;
    if (sat) {                                   // rare: a few hundred pixels of a CCD
        const int x = (int)(p % nx), y = (int)(p / nx);
        const int ymid = ny / 2;
        const int half = (midline_stop && y >= ymid) ? 1 : 0;
        const int yl = half ? y - ymid : y;
        atomicMin(&span[4 * x + 2 * half], yl);
        atomicMax(&span[4 * x + 2 * half + 1], yl);
    }
}

// BleedCharge.__call__ (bleed_trails.py:117-152): returns true once the excess is used up
__device__ __forceinline__ bool bleed_into(double* __restrict__ c, int64_t stride, int n, int ypix, double full_well, double& excess)
{
    if (ypix >= 0 && ypix < n) {
        const double room = full_well - c[(int64_t)ypix * stride];
        const double b = room < excess ? room : excess;
        c[(int64_t)ypix * stride] = c[(int64_t)ypix * stride] + b;
        excess = excess - b;
    } else if (ypix < 0) {
        excess = excess - (full_well < excess ? full_well : excess);      // leaves through the serial register
    }
    return excess == 0.0;
}

// one thread per channel (a column, or half a column with the midline stop); neighbouring threads walk neighbouring
// columns, so every step of the walk is one coalesced row access
__global__ __launch_bounds__(256) void k_readout_bleed(double* __restrict__ image, const unsigned char* __restrict__ flags,
                                                       const int* __restrict__ span, int nx, int ny, double full_well,
                                                       int midline_stop)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_half = midline_stop ? 2 : 1;
    if (t >= nx * n_half) return;
    const int x = t % nx, half = t / nx;
    const int ymid = ny / 2;
    const int ylo = (midline_stop && half == 1) ? ymid : 0;
    const int n = midline_stop ? (half == 0 ? ymid : ny - ymid) : ny;
    double* c = image + (int64_t)ylo * nx + x;
    const unsigned char* f = flags + (int64_t)ylo * nx + x;
    // runs are found on the ORIGINAL flags: only the rows between the first and the last saturated pixel need a look
    int y = span[4 * x + 2 * half];
    const int y_last = span[4 * x + 2 * half + 1];
    while (y <= y_last) {
        // the way to the next saturated row, eight rows' flags at a time (independent loads: the walk used to wait for every
        // single byte before it asked for the next)
        unsigned char fl[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) fl[q] = (y + q <= y_last) ? f[(int64_t)(y + q) * nx] : (unsigned char)0;
        int skip = 0;
        while (skip < 8 && !fl[skip]) ++skip;
        y += skip;
        if (skip == 8) continue;
        const int y0 = y;
        while (y < n && f[(int64_t)y * nx]) ++y;
        const int y1 = y;
        double excess = 0.0;
        for (int k = y0; k < y1; ++k) excess = excess + c[(int64_t)k * nx];
        excess = excess - (double)(y1 - y0) * full_well;
        for (int k = y0; k < y1; ++k) c[(int64_t)k * nx] = full_well;
        const int reach = y0 > n - y1 ? y0 : n - y1;
        for (int dy = 0; dy < reach; ++dy) {
            if (bleed_into(c, nx, n, y0 - dy - 1, full_well, excess)) break;
            if (bleed_into(c, nx, n, y1 + dy, full_well, excess)) break;
        }
    }
}

// e-image pixel read out at position (u, v) of amp a's imaging section, in ADU (float32 like the reference's arrays)
__device__ __forceinline__ float amp_adu(const double* __restrict__ image, int nx, const ims_readout_t& ro, int a, int u, int v)
{
    const ims_amp_t& A = ro.amps[a];
    const int sx = A.flip_x ? ro.seg_w - 1 - u : u;
    const int sy = A.flip_y ? ro.seg_h - 1 - v : v;
    const float e = (float)image[(int64_t)(A.y0 + sy) * nx + (A.x0 + sx)];
    return e / A.gain;
}

// grid (raw_w / 64, raw_h / 4, n_amps), block (64, 4)
// grid (raw_w / 64, raw_h / 4), block (64, 4): a thread forms position (rx, ry) of ALL amplifiers' raw segments -- crosstalk makes every
// amplifier's pixel there a sum over the sixteen pixels at that position, which were read sixteen times (once per output amplifier:
// 2.1 GB for a 131-MB image) and are read once now; the sums are the same sums (ascending source amplifier, zero coefficients skipped)
__global__ __launch_bounds__(256) void k_readout_segments(const double* __restrict__ image, int nx, const ims_readout_t ro,
                                                          float* __restrict__ seg)
{
    const int rx = blockIdx.x * 64 + threadIdx.x, ry = blockIdx.y * 4 + threadIdx.y;
    if (rx >= ro.raw_w || ry >= ro.raw_h) return;
    const int u = rx - ro.data_x0, v = ry - ro.data_y0;
    const bool inside = u >= 0 && u < ro.seg_w && v >= 0 && v < ro.seg_h;
    float e[IMS_MAX_AMPS];
#pragma unroll
    for (int a = 0; a < IMS_MAX_AMPS; ++a) e[a] = (inside && a < ro.n_amps) ? amp_adu(image, nx, ro, a, u, v) : 0.0f;
#pragma unroll
    for (int a = 0; a < IMS_MAX_AMPS; ++a) {
        if (a >= ro.n_amps) break;
        float out = 0.0f;
        if (inside) {
            out = e[a];
            if (ro.has_xtalk) {
                float sum = 0.0f;
#pragma unroll
                for (int j = 0; j < IMS_MAX_AMPS; ++j) {
                    if (j >= ro.n_amps) break;
                    const float x = ro.xtalk[a * IMS_MAX_AMPS + j];
                    if (x != 0.0f) sum = sum + x * e[j];          // a zero coefficient adds exactly nothing
                }
                out = out + sum;
            }
        }
        seg[((int64_t)a * ro.raw_h + ry) * ro.raw_w + rx] = out;
    }
}

// grid (raw_w / 64, raw_h / 4, n_amps), block (64, 4): a wavefront is 64 neighbouring columns of one row, so every tap
// of the parallel direction is one coalesced 256-B row access and the four rows of a workgroup share their taps in L1;
// no integer division anywhere.
// NB > 0: the band width is known at compile time (the reference's ntransfers = 20: 21 taps); pixels with a full
// set of taps take an unrolled path whose 2 x 21 loads are all in flight before the first use.
template <int NB>
__global__ __launch_bounds__(256) void k_readout_cte(const float* __restrict__ src, float* __restrict__ dst, int raw_w, int raw_h,
                                                     const double* __restrict__ band, int n_band, int axis)
{
    const int rx = blockIdx.x * 64 + threadIdx.x, ry = blockIdx.y * 4 + threadIdx.y;
    // serial direction: every lane has a row of weights of its own (its column's) -- the workgroup's 64 rows of weights are one
    // contiguous piece of the band matrix, staged through LDS once instead of 21 scattered 8-byte loads per lane and row
    __shared__ double wl[64 * (NB > 0 ? NB : 1)];
    const bool staged = NB > 0 && axis == 1;
    if (staged) {
        const int i0 = blockIdx.x * 64;
        for (int e = threadIdx.y * 64 + threadIdx.x; e < 64 * NB; e += 256)
            wl[e] = (i0 + e / NB < raw_w) ? band[(int64_t)i0 * NB + e] : 0.0;
        __syncthreads();
    }
    if (rx >= raw_w || ry >= raw_h) return;
    const int p = ((int)blockIdx.z * raw_h + ry) * raw_w + rx;
    const int i = axis == 0 ? ry : rx;
    const int step = axis == 0 ? raw_w : 1;
    const int dmax = i < n_band - 1 ? i : n_band - 1;
    const double* w = band + i * n_band;
    const double* ws = wl + threadIdx.x * (NB > 0 ? NB : 1);
    double acc = 0.0;
    if (NB > 0 && i >= NB - 1) {
        float v[NB > 0 ? NB : 1];
        double ww[NB > 0 ? NB : 1];
#pragma unroll
        for (int d = 0; d < NB; ++d) v[d] = src[p - d * step];
        if (staged) {
#pragma unroll
            for (int d = 0; d < NB; ++d) ww[d] = ws[d];
        } else {
#pragma unroll
            for (int d = 0; d < NB; ++d) ww[d] = w[d];
        }
#pragma unroll
        for (int d = NB - 1; d >= 0; --d) acc = acc + ww[d] * (double)v[d];
    } else if (staged) {
        for (int d = dmax; d >= 0; --d) acc = acc + ws[d] * (double)src[p - d * step];
    } else {
        for (int d = dmax; d >= 0; --d) acc = acc + w[d] * (double)src[p - d * step];
    }
    dst[p] = (float)acc;
}

// The read-noise deviates of pixels 2 m and 2 m + 1 of an amplifier are the two Gaussians of ONE counter block: a thread forms the
// block once and finishes both pixels (segments of an even number of pixels; the single-pixel kernel below did the block twice).
__global__ __launch_bounds__(256) void k_readout_finish_pairs(const float* __restrict__ seg, const ims_readout_t ro, uint64_t seed,
                                                              int32_t* __restrict__ out)
{
    const int64_t per = (int64_t)ro.raw_w * ro.raw_h;
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // pair number over all amplifiers
    if (2 * m >= per * ro.n_amps) return;
    const int64_t p = 2 * m;
    const int a = (int)(p / per);
    const int64_t q = p - (int64_t)a * per;                                 // even
    typedef float fvec2 __attribute__((ext_vector_type(2)));
    typedef int ivec2 __attribute__((ext_vector_type(2)));
    const fvec2 sv = *(const fvec2*)(seg + p);
    Rng r;
    rng_reset(r);
    rng_block(r, seed, READOUT_ID_BASE + a, q >> 1, 0u);
    double g0, g1;
    gauss_words(r.w[0], r.w[1], g0, g1);
    float v0 = sv.x + ro.amps[a].bias_level, v1 = sv.y + ro.amps[a].bias_level;
    v0 = v0 + (float)((double)ro.amps[a].read_noise * g0);
    v1 = v1 + (float)((double)ro.amps[a].read_noise * g1);
    ivec2 o;
    o.x = (int32_t)v0; o.y = (int32_t)v1;
    *(ivec2*)(out + p) = o;
}

__global__ __launch_bounds__(256) void k_readout_finish(const float* __restrict__ seg, const ims_readout_t ro, uint64_t seed,
                                                        int32_t* __restrict__ out)
{
    const int64_t per = (int64_t)ro.raw_w * ro.raw_h;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= per * ro.n_amps) return;
    const int a = (int)(p / per);
    const int64_t q = p - (int64_t)a * per;
    float v = seg[p] + ro.amps[a].bias_level;
    Rng r;
    rng_reset(r);
    rng_block(r, seed, READOUT_ID_BASE + a, q >> 1, 0u);
    double g0, g1;
    gauss_words(r.w[0], r.w[1], g0, g1);
    v = v + (float)((double)ro.amps[a].read_noise * ((q & 1) ? g1 : g0));
    out[p] = (int32_t)v;
}

extern "C" {

static int check_readout(const ims_readout_t* ro)
{
    if (!ro) return set_err(IMS_ERR_ARG, "readout descriptor is NULL");
    if (ro->n_amps < 1 || ro->n_amps > IMS_MAX_AMPS) return set_err(IMS_ERR_ARG, "n_amps out of range");
    if (ro->seg_w < 1 || ro->seg_h < 1 || ro->data_x0 < 0 || ro->data_y0 < 0 || ro->data_x0 + ro->seg_w > ro->raw_w ||
        ro->data_y0 + ro->seg_h > ro->raw_h)
        return set_err(IMS_ERR_ARG, "imaging section does not fit the raw segment");
    for (int a = 0; a < ro->n_amps; ++a)
        if (!(ro->amps[a].gain > 0.0f)) return set_err(IMS_ERR_ARG, "amplifier gain must be positive");
    return IMS_OK;
}

int ims_readout_bleed(double* image_dev, unsigned char* flags_dev, int32_t nx, int32_t ny, double full_well,
                      int32_t midline_stop, void* stream)
{
    if (!image_dev || !flags_dev) return set_err(IMS_ERR_ARG, "image / flags is NULL");
    if (nx < 1 || ny < 1) return set_err(IMS_ERR_ARG, "empty image");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)nx * ny;
    int* span = (int*)(flags_dev + ((n + 15) / 16) * 16);        // the tail of the scratch: 4 ints per column
    hipLaunchKernelGGL(k_readout_span_init, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, span, nx);
    hipLaunchKernelGGL(k_readout_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, image_dev, flags_dev, span, nx, ny,
                       full_well, midline_stop ? 1 : 0);
    const int threads = nx * (midline_stop ? 2 : 1);
    hipLaunchKernelGGL(k_readout_bleed, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, image_dev, flags_dev, span, nx, ny,
                       full_well, midline_stop ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_readout_segments(const double* image_dev, int32_t nx, int32_t ny, const ims_readout_t* ro, float* seg_dev, void* stream)
{
    if (int e = check_readout(ro)) return e;
    if (!image_dev || !seg_dev) return set_err(IMS_ERR_ARG, "image / segments is NULL");
    for (int a = 0; a < ro->n_amps; ++a)
        if (ro->amps[a].x0 < 0 || ro->amps[a].y0 < 0 || ro->amps[a].x0 + ro->seg_w > nx || ro->amps[a].y0 + ro->seg_h > ny)
            return set_err(IMS_ERR_ARG, "amplifier section outside the e-image");
    hipLaunchKernelGGL(k_readout_segments, dim3((unsigned)((ro->raw_w + 63) / 64), (unsigned)((ro->raw_h + 3) / 4), 1u),
                       dim3(64, 4), 0, (hipStream_t)stream, image_dev, nx, *ro, seg_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_readout_cte(const float* src_dev, float* dst_dev, const ims_readout_t* ro, const double* band_dev, int32_t n_band,
                    int32_t axis, void* stream)
{
    if (int e = check_readout(ro)) return e;
    if (!src_dev || !dst_dev || !band_dev) return set_err(IMS_ERR_ARG, "src / dst / band is NULL");
    if (src_dev == dst_dev) return set_err(IMS_ERR_ARG, "ims_readout_cte is out of place: src and dst must differ");
    if (n_band < 1 || (axis != 0 && axis != 1)) return set_err(IMS_ERR_ARG, "n_band / axis out of range");
    if ((int64_t)ro->raw_w * ro->raw_h * ro->n_amps >= (1ll << 31)) return set_err(IMS_ERR_ARG, "raw segments too large");
    const dim3 grid((unsigned)((ro->raw_w + 63) / 64), (unsigned)((ro->raw_h + 3) / 4), (unsigned)ro->n_amps);
    if (n_band == 21)
        hipLaunchKernelGGL(k_readout_cte<21>, grid, dim3(64, 4), 0, (hipStream_t)stream, src_dev, dst_dev, ro->raw_w, ro->raw_h,
                           band_dev, n_band, axis);
    else
        hipLaunchKernelGGL(k_readout_cte<0>, grid, dim3(64, 4), 0, (hipStream_t)stream, src_dev, dst_dev, ro->raw_w, ro->raw_h,
                           band_dev, n_band, axis);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_readout_finish(const float* seg_dev, const ims_readout_t* ro, uint64_t seed, int32_t* out_dev, void* stream)
{
    if (int e = check_readout(ro)) return e;
    if (!seg_dev || !out_dev) return set_err(IMS_ERR_ARG, "segments / output is NULL");
    const int64_t n = (int64_t)ro->raw_w * ro->raw_h * ro->n_amps;
    if ((((int64_t)ro->raw_w * ro->raw_h) & 1) == 0 && (((uintptr_t)seg_dev | (uintptr_t)out_dev) & 7u) == 0)
        hipLaunchKernelGGL(k_readout_finish_pairs, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg_dev, *ro,
                           seed, out_dev);
    else
        hipLaunchKernelGGL(k_readout_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg_dev, *ro, seed,
                           out_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
