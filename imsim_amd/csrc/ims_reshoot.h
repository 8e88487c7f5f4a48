// ims_reshoot.h -- section of the one translation unit (imsim_hip.hip): FFT-drawn stamps turned into photons, run through the
// photon operators and binned back (stamp.fft_photon_ops behind stamp.fft_reshoot; imsim/stamp.py:493-499, GalSim's
// drawImage(method='fft', photon_ops=...) -> PhotonArray.makeFromImage -> operators -> accumulation without a sensor).
//
// The stage sits between the inverse transforms and the spike / finish steps: it reads the real-space buffer of a batch (raw or
// scaled, rbuf_value) and writes a second buffer of the same layout, zero outside every object's stamp rectangle.
//
// Photons of an object (makeFromImage): the stamp's pixels in row-major order, a pixel of value v spawns N = 0 photons if v == 0,
// 1 if |v| <= max_flux, else ceil(|v| / max_flux), of flux v / N each.  Photon k of an object -- k the exclusive prefix of N over the
// stamp plus the index inside the pixel -- draws one Philox block (seed, obj_id, k, SLOT_RESHOOT): w0 the wavelength (shoot's
// lookup), w1 / w2 the place inside the pixel, x = px + (w01(w1) - 0.5), y = py + (w01(w2) - 0.5) in CCD pixels; then
// run_ops<CHAIN, LAYOUT> on the object's ims_object_t row with photon number k.
//
// Binning: flux == 0 is lost; pixel (floor(x + 0.5), floor(y + 0.5)); outside the stamp rectangle is lost.  The deposit is the INTEGER
// llrint(flux * 2^32), added with 64-bit integer atomics; a last pass turns the sums into doubles (x 2^-32) in place.  Every sum is
// an integer sum and every deviate is addressed by (object, k): the result does not depend on the grid size, the run length or the
// order of arrival.
//
// Work distribution: a grid is cut into tiles of RS_TILE = 1024 grid points (grids are powers of two from 32: a tile never straddles
// two objects).  k_reshoot_count sums N per tile, k_reshoot_scan turns the tile sums into an exclusive prefix over ALL tiles of the
// batch (one workgroup; the last entry is the batch's photon total), k_fft_reshoot shoots: a fixed grid of workgroups strides over
// RUNS of IMS_RESHOOT_RUN consecutive photon numbers of that prefix up to the total, which it reads from the device -- nothing is
// read back.  A workgroup finds the first tile of its run by bisection (scalar operands), forms the tile's inclusive per-pixel scan
// in LDS (8 KB), and each lane finds its pixel there by bisection.  A bright core pixel holds millions of photons: its runs all
// find the same tile, one pixel each.  Deposits near the first pixel of a tile visit go to a 16 x 16 LDS window of int64 sums
// first (most photons land in the pixel they came from or beside it) and from there with one global atomic per cell.
//
// Kernels: k_reshoot_count, k_reshoot_scan, k_fft_reshoot<CHAIN, LAYOUT> (it runs no PSF: no PSF variants), k_reshoot_convert.
// Entry points: ims_fft_reshoot_work_bytes, ims_fft_reshoot.
#pragma once

constexpr int RS_TILE = 1024;               // grid points per tile: four per thread of the counting workgroup
constexpr int RS_WIN = 16;                  // side of the LDS deposit window
constexpr int64_t RS_RUN = IMS_RESHOOT_RUN; // photon numbers per run
constexpr int RS_GRID = 2048;               // workgroups of the shooting launch: two rounds of four on each of 256 CUs
constexpr int RS_SCAN_THREADS = 1024;

// makeFromImage's photon count of a pixel (a value that is not finite spawns none)
__device__ __forceinline__ int64_t reshoot_count(double v, double max_flux)
{
    if (v == 0.0) return 0;
    const double a = fabs(v);
    if (a <= max_flux) return 1;
    const double q = ceil(ddiv(a, max_flux));
    if (!(q < 0x1.0p62)) return 0;
    return (int64_t)q;
}

// the value of grid point `local` of object o as the image holds it; 0 outside the stamp rectangle (k_fft_finish's test)
__device__ __forceinline__ double reshoot_pixel(const ims_fft_object_t& o, const double* __restrict__ rbuf, int64_t local, bool raw,
                                                int& px, int& py)
{
    int iy, ix;
    row_col(local, o.nfft, iy, ix);
    px = o.x0 + ix; py = o.y0 + iy;
    if (px < o.stamp_xmin || px > o.stamp_xmax || py < o.stamp_ymin || py > o.stamp_ymax) return 0.0;
    return rbuf_value(rbuf, o.r_offset + local, raw, inv_n2(o.nfft));
}

__device__ __forceinline__ long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one workgroup per tile: tile_count[t] = sum of N over the tile's 1024 grid points
__global__ __launch_bounds__(256) void k_reshoot_count(const ims_fft_object_t* __restrict__ objs, int64_t n_objects,
                                                       const int64_t* __restrict__ r_prefix, const double* __restrict__ rbuf, int raw,
                                                       double max_flux, int64_t* __restrict__ tile_count)
{
    __shared__ long long part[4];
    const int64_t t = blockIdx.x;
    const int64_t first = t * RS_TILE;
    const int64_t oi = find_object(r_prefix, n_objects, first);
    const ims_fft_object_t& o = objs[oi];
    const int64_t base = first - r_prefix[oi] + 4 * (int64_t)threadIdx.x;
    long long n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int px, py;
        n += reshoot_count(reshoot_pixel(o, rbuf, base + q, raw != 0, px, py), max_flux);
    }
    n = wave_sum_ll(n);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[t] = ((part[0] + part[1]) + part[2]) + part[3];
}

// one workgroup: scan[0 .. n_tiles] = exclusive prefix of the tile counts, in place; scan[n_tiles] = the photon total
__global__ __launch_bounds__(RS_SCAN_THREADS) void k_reshoot_scan(int64_t* __restrict__ scan, int64_t n_tiles)
{
    __shared__ long long part[RS_SCAN_THREADS];
    const int tid = (int)threadIdx.x;
    const int64_t chunk = (n_tiles + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS;
    const int64_t a = tid * chunk < n_tiles ? tid * chunk : n_tiles;
    const int64_t b = a + chunk < n_tiles ? a + chunk : n_tiles;
    long long s = 0;
    for (int64_t t = a; t < b; ++t) s += scan[t];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < RS_SCAN_THREADS; off <<= 1) {
        const long long add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    long long run = part[tid] - s;
    for (int64_t t = a; t < b; ++t) {
        const long long c = scan[t];
        scan[t] = run;
        run += c;
    }
    if (tid == RS_SCAN_THREADS - 1) scan[n_tiles] = part[tid];
}

template <int CHAIN, unsigned long long LAYOUT>
__global__ __launch_bounds__(256, (CHAIN == 1) ? IMS_CHAIN_WAVES : IMS_FUSED_WAVES) void k_fft_reshoot(
    const ims_render_params_t P, const ims_fft_object_t* __restrict__ fobjs, const ims_object_t* __restrict__ pobjs, int64_t n_objects,
    const int64_t* __restrict__ r_prefix, int64_t n_tiles, const double* __restrict__ rbuf, int raw, double max_flux,
    const int64_t* __restrict__ scan, unsigned long long* __restrict__ img, const ims_photons_t pool,
    const int64_t* __restrict__ pool_offset, int32_t* __restrict__ land_out, int pool_stage)
{
    __shared__ long long incl[RS_TILE];
    __shared__ unsigned long long win[RS_WIN * RS_WIN];
    __shared__ long long part[4];
    const int tid = (int)threadIdx.x;
    const int64_t total = scan[n_tiles];
    const int64_t n_runs = (total + RS_RUN - 1) / RS_RUN;
    // (run, g, t and oi are uniform over the workgroup: every barrier below is reached by all 256 threads)
    for (int64_t run = blockIdx.x; run < n_runs; run += gridDim.x) {
        int64_t g = run * RS_RUN;
        const int64_t g1 = g + RS_RUN < total ? g + RS_RUN : total;
        int64_t t = find_object(scan, n_tiles, g);          // scan[t] <= g < scan[t + 1]
        int64_t oi = -1, o_end = 0;
        while (g < g1) {
            const int64_t first = t * RS_TILE;
            if (first >= o_end) { oi = find_object(r_prefix, n_objects, first); o_end = r_prefix[oi + 1]; }
            const ims_fft_object_t& fo = fobjs[oi];
            const ims_object_t& po = pobjs[oi];
            const int64_t o_begin = r_prefix[oi];
            const int64_t t_begin = scan[t], t_end = scan[t + 1];
            const int64_t ga = g, gb = t_end < g1 ? t_end : g1;
            const int64_t k_base = scan[o_begin / RS_TILE];  // photons of the batch before this object's first
            // the tile's inclusive per-pixel scan: four consecutive grid points per thread, the wavefronts in turn
            {
                long long c[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int px, py;
                    c[q] = reshoot_count(reshoot_pixel(fo, rbuf, first - o_begin + 4 * tid + q, raw != 0, px, py), max_flux);
                    s += c[q];
                }
                long long inc = s;                           // inclusive scan of s over the wavefront
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const long long up = __shfl_up(inc, off, 64);
                    if ((tid & 63) >= off) inc += up;
                }
                if ((tid & 63) == 63) part[tid >> 6] = inc;
                __syncthreads();
                long long before = inc - s;
                for (int w = 0; w < (tid >> 6); ++w) before += part[w];
#pragma unroll
                for (int q = 0; q < 4; ++q) { before += c[q]; incl[4 * tid + q] = before; }
            }
            win[tid] = 0ull;
            __syncthreads();
            // the deposit window: centred on the pixel of the visit's first photon (every lane the same bisection)
            int wx0, wy0;
            {
                const long long q0 = ga - t_begin;
                int lo = 0, hi = RS_TILE - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (incl[mid] > q0) hi = mid; else lo = mid + 1; }
                int iy, ix;
                row_col(first - o_begin + lo, fo.nfft, iy, ix);
                wx0 = ix - RS_WIN / 2; wy0 = iy - RS_WIN / 2;
            }
            for (int64_t gl = ga + tid; gl < gb; gl += 256) {
                const long long q = gl - t_begin;
                int lo = 0, hi = RS_TILE - 1;                // the first grid point whose inclusive count exceeds q
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (incl[mid] > q) hi = mid; else lo = mid + 1; }
                const long long excl = lo > 0 ? incl[lo - 1] : 0;
                const long long n_here = incl[lo] - excl;
                int px, py;
                const double v = reshoot_pixel(fo, rbuf, first - o_begin + lo, raw != 0, px, py);
                const int64_t k = gl - k_base;
                Photon ph;
                Rng rng;
                rng_reset(rng);
                rng_block(rng, P.seed, po.obj_id, k, SLOT_RESHOOT);
                double wl = po.sed_wave;
                if (po.sed_table >= 0) wl = lin_lookup(P.sed, po.sed_table, w01(rng.w[0]));
                ph.x = (double)px + (w01(rng.w[1]) - 0.5);
                ph.y = (double)py + (w01(rng.w[2]) - 0.5);
                ph.flux = n_here == 1 ? v : ddiv(v, (double)n_here);
                ph.dxdz = 0.0; ph.dydz = 0.0; ph.wl = wl; ph.pu = 0.0; ph.pv = 0.0; ph.t = 0.0;
                int64_t slot = -1;
                if (pool_stage != 0) {
                    slot = pool_offset[oi] + k;
                    if (slot >= pool_offset[oi + 1] || slot >= pool.n) slot = -1;
                }
                if (pool_stage == 1 && slot >= 0) {
                    pool.x[slot] = ph.x; pool.y[slot] = ph.y; pool.flux[slot] = ph.flux; pool.dxdz[slot] = ph.dxdz; pool.dydz[slot] = ph.dydz;
                    pool.wavelength[slot] = ph.wl;
                    if (pool.pupil_u) { pool.pupil_u[slot] = ph.pu; pool.pupil_v[slot] = ph.pv; pool.time[slot] = ph.t; }
                    if (pool.obj_index) pool.obj_index[slot] = (int32_t)oi;
                }
                run_ops<CHAIN, LAYOUT>(P, po, k, rng, ph);
                if (pool_stage == 2 && slot >= 0) {
                    pool.x[slot] = ph.x; pool.y[slot] = ph.y; pool.flux[slot] = ph.flux; pool.dxdz[slot] = ph.dxdz; pool.dydz[slot] = ph.dydz;
                    pool.wavelength[slot] = ph.wl;
                    if (pool.pupil_u) { pool.pupil_u[slot] = ph.pu; pool.pupil_v[slot] = ph.pv; pool.time[slot] = ph.t; }
                    if (pool.obj_index) pool.obj_index[slot] = (int32_t)oi;
                }
                int32_t land = -1;
                if (ph.flux != 0.0) {
                    const double fx = floor(ph.x + 0.5), fy = floor(ph.y + 0.5);
                    // (compared as doubles: a position that is not a number, or beyond an int, is outside)
                    if (fx >= (double)fo.stamp_xmin && fx <= (double)fo.stamp_xmax && fy >= (double)fo.stamp_ymin && fy <= (double)fo.stamp_ymax) {
                        const int gx = (int)fx - fo.x0, gy = (int)fy - fo.y0;        // inside the grid: the host checks stamp <= grid
                        const unsigned long long d = (unsigned long long)__double2ll_rn(ph.flux * 0x1.0p32);
                        land = gy * fo.nfft + gx;
                        const int wx = gx - wx0, wy = gy - wy0;
                        if (wx >= 0 && wx < RS_WIN && wy >= 0 && wy < RS_WIN) atomicAdd(&win[wy * RS_WIN + wx], d);
                        else atomicAdd(img + (fo.r_offset + land), d);
                    }
                }
                if (land_out != nullptr && slot >= 0) land_out[slot] = land;
            }
            __syncthreads();
            {
                const unsigned long long d = win[tid];
                const int gx = wx0 + (tid & (RS_WIN - 1)), gy = wy0 + tid / RS_WIN;
                if (d != 0ull) atomicAdd(img + (fo.r_offset + (int64_t)gy * fo.nfft + gx), d);   // (non-zero: a deposit put it there, inside the stamp)
            }
            __syncthreads();
            g = gb;
            if (g < g1) {
                ++t;
                if (scan[t + 1] <= g) t = find_object(scan, n_tiles, g);     // empty tiles in between
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_reshoot_convert(double* __restrict__ out, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const long long s = __double_as_longlong(out[i]);
        out[i] = (double)s * 0x1.0p-32;
    }
}

extern "C" {

int64_t ims_fft_reshoot_work_bytes(int64_t n_pix)
{
    if (n_pix < 0 || n_pix % RS_TILE != 0) return (int64_t)set_err(IMS_ERR_ARG, "fft_reshoot: n_pix must be a non-negative multiple of 1024");
    return (n_pix / RS_TILE + 1) * (int64_t)sizeof(int64_t);
}

int ims_fft_reshoot(const ims_fft_params_t* fft_params, const ims_render_params_t* render_params, const ims_fft_object_t* fft_objects_dev,
                    const ims_fft_object_t* fft_objects_host, const ims_object_t* photon_objects_dev, int64_t n_objects,
                    const int64_t* r_prefix_dev, int64_t n_pix, const double* rbuf_in, int32_t raw, double max_flux, void* work_dev,
                    double* out_dev, const ims_photons_t* pool_out, const int64_t* pool_offset_dev, int32_t* land_dev,
                    int32_t pool_stage, int32_t grid, void* stream)
{
    if (!fft_params || !render_params) return set_err(IMS_ERR_ARG, "fft_reshoot: params is NULL");
    if (n_objects < 0 || n_pix < 0) return set_err(IMS_ERR_ARG, "fft_reshoot: negative count");
    if (!(max_flux > 0.0) || !(max_flux < 0x1.0p31)) return set_err(IMS_ERR_ARG, "fft_reshoot: max_flux must be positive (and below 2^31)");
    if (pool_stage < 0 || pool_stage > 2) return set_err(IMS_ERR_ARG, "fft_reshoot: pool_stage must be 0, 1 or 2");
    if (raw != 0 && raw != 1) return set_err(IMS_ERR_ARG, "fft_reshoot: raw must be 0 or 1");
    if (grid < 0 || grid > 65535) return set_err(IMS_ERR_ARG, "fft_reshoot: grid must be 0 (the library's) or 1 .. 65535 workgroups");
    if (pool_stage != 0) {
        if (!pool_out || !pool_offset_dev) return set_err(IMS_ERR_ARG, "fft_reshoot: pool_stage without pool_out / pool_offset");
        if (pool_out->n < 1 || pool_out->converted) return set_err(IMS_ERR_ARG, "fft_reshoot: the pool is too small (n < 1) or a converted pool");
        if (!pool_out->x || !pool_out->y || !pool_out->flux || !pool_out->dxdz || !pool_out->dydz || !pool_out->wavelength)
            return set_err(IMS_ERR_ARG, "fft_reshoot: the pool lacks one of x, y, flux, dxdz, dydz, wavelength");
        if (pool_out->pupil_u && (!pool_out->pupil_v || !pool_out->time)) return set_err(IMS_ERR_ARG, "fft_reshoot: pupil_u without pupil_v / time");
    } else if (land_dev) return set_err(IMS_ERR_ARG, "fft_reshoot: land_dev is indexed like the pool (pool_stage 1 or 2)");
    if (n_objects == 0 || n_pix == 0) return IMS_OK;
    if (!fft_objects_dev || !fft_objects_host || !photon_objects_dev || !r_prefix_dev || !rbuf_in || !work_dev || !out_dev)
        return set_err(IMS_ERR_ARG, "fft_reshoot: NULL argument");
    if (rbuf_in == out_dev) return set_err(IMS_ERR_ARG, "fft_reshoot: the output buffer is a second buffer");
    if (n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "fft_reshoot: too many objects for one call");
    int64_t at = 0;
    for (int64_t i = 0; i < n_objects; ++i) {
        const ims_fft_object_t& o = fft_objects_host[i];
        const int64_t n2 = (int64_t)o.nfft * o.nfft;
        if (o.nfft < 32 || o.nfft > 32768 || n2 % RS_TILE != 0) return set_err(IMS_ERR_ARG, "fft_reshoot: nfft must be 32 .. 32768 with nfft^2 a multiple of 1024");
        if (o.r_offset != at) return set_err(IMS_ERR_ARG, "fft_reshoot: r_offset is not the prefix sum of nfft^2");
        if (!(fabs(o.flux) < 0x1.0p31)) return set_err(IMS_ERR_ARG, "fft_reshoot: an object's |flux| is 2^31 e- or more (the integer sums hold less)");
        if (o.stamp_xmin > o.stamp_xmax || o.stamp_ymin > o.stamp_ymax || o.stamp_xmin < o.x0 || o.stamp_ymin < o.y0 ||
            (int64_t)o.stamp_xmax > (int64_t)o.x0 + o.nfft - 1 || (int64_t)o.stamp_ymax > (int64_t)o.y0 + o.nfft - 1)
            return set_err(IMS_ERR_ARG, "fft_reshoot: a stamp rectangle is empty or not inside its grid");
        at += n2;
    }
    if (at != n_pix) return set_err(IMS_ERR_ARG, "fft_reshoot: n_pix is not the sum of nfft^2");
    int rc = check_params(render_params);
    if (rc) return rc;
    ims_render_params_t ops_only = *render_params;       // the kernel is chosen by chain and optics layout alone
    ops_only.n_psf = 0;
    const PhotonVariant v = select_photon_variant(&ops_only, 2);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_tiles = n_pix / RS_TILE;
    if (n_tiles > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "fft_reshoot: too many grid points for one call");
    int64_t* scan = (int64_t*)work_dev;
    ims_photons_t pool;
    memset(&pool, 0, sizeof(pool));
    if (pool_stage != 0) pool = *pool_out;
    HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)n_pix * sizeof(double), st));
    hipLaunchKernelGGL(k_reshoot_count, dim3((unsigned)n_tiles), dim3(256), 0, st, fft_objects_dev, n_objects, r_prefix_dev, rbuf_in,
                       (int)raw, max_flux, scan);
    hipLaunchKernelGGL(k_reshoot_scan, dim3(1), dim3(RS_SCAN_THREADS), 0, st, scan, n_tiles);
    const unsigned wgs = grid > 0 ? (unsigned)grid : (unsigned)RS_GRID;
    bool launched = false;
#define IMS_TRY_RESHOOT(C, L) if (!launched && v.chain == C && v.layout == L) { launched = true; \
        hipLaunchKernelGGL((k_fft_reshoot<C, L>), dim3(wgs), dim3(256), 0, st, *render_params, fft_objects_dev, photon_objects_dev, n_objects, \
                           r_prefix_dev, n_tiles, rbuf_in, (int)raw, max_flux, (const int64_t*)scan, (unsigned long long*)out_dev, pool, \
                           pool_offset_dev, land_dev, (int)pool_stage); }
    IMS_TRY_RESHOOT(0, 0ull) IMS_TRY_RESHOOT(0, IMS_LAYOUT_PERTURBED) IMS_TRY_RESHOOT(1, 0ull) IMS_TRY_RESHOOT(1, IMS_LAYOUT_RUBIN_LIKE)
#undef IMS_TRY_RESHOOT
    if (!launched) {
        char msg[160];
        snprintf(msg, sizeof(msg), "fft_reshoot: no kernel <CHAIN %d, LAYOUT 0x%llx>", v.chain, v.layout);
        return set_err(IMS_ERR_UNSUPPORTED, msg);
    }
    hipLaunchKernelGGL(k_reshoot_convert, dim3(grid_for_pool(n_pix)), dim3(256), 0, st, out_dev, n_pix);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
