// ims_fft_branch.h -- section of the one translation unit (imsim_hip.hip): the FFT branch (bright objects drawn in k-space).
// (ims_fft.h is the device header of the k-space profiles these kernels evaluate.)
//
// Kernels: k_fft_kspace_fill (the half spectra, walked in spans: walk_span), k_fft_spike_table, k_fft_bbox, k_fft_spikes,
// k_fft_spikes_stream, k_fft_spikes_arms (DiffractionFFT), k_fft_finish (clip, Poisson noise, add to the CCD); and, further down
// beside the entry points that launch them, k_scale (ahead of the plan cache) and k_fill_bbox (inside the extern "C" block, ahead
// of ims_fft_spike_table: it keeps its unmangled name).
// Host: the hipFFT plan cache (fft_plan_get, fft_inverse_impl; the plans themselves are in ims_host.h), fft_span.
// Entry points: ims_fft_warm, ims_fft_inverse, ims_fft_inverse_raw, ims_fft_kspace_fill, ims_fft_spike_table, ims_fft_spikes,
// ims_fft_spikes_listed, ims_fft_finish.
#pragma once

// ---------------- FFT branch ----------------
// row and column of element `local` of a grid of row length `len` (FFT sizes are powers of two: a shift; half spectra -- len =
// nfft / 2 + 1 -- and anything else: a 32-bit division, the grids hold fewer than 2^31 elements)
__device__ __forceinline__ void row_col(int64_t local, int len, int& row, int& col)
{
    const uint32_t l = (uint32_t)local, n = (uint32_t)len;
    if ((n & (n - 1u)) == 0u) { const int sh = 31 - __clz((int)n); row = (int)(l >> sh); col = (int)(l & (n - 1u)); }
    else { row = (int)(l / n); col = (int)(l - (uint32_t)row * n); }
}

// The elementwise kernels of the FFT branch walk the back-to-back grids of their objects in SPANS: a workgroup owns `span` consecutive
// elements (a multiple of 256, fft_span below), a wavefront 64 consecutive ones per pass.  The object of a wavefront's elements is
// found ONCE per span (a bisection with scalar operands) and then only moved along when the wavefront's first element passes the
// object's end; a wavefront that lies inside one object -- all of them but the few on a boundary -- calls the body with a UNIFORM object
// number, so that the object's row and its prefix entry come by scalar loads.  (A grid-stride loop used to bisect in every pass: 13
// dependent loads before the first useful one, `k_fft_finish` waited 67 % of its wave-cycles and moved 0.26 TB/s, round 6.)
template <class Body>
__device__ __forceinline__ void walk_span(const int64_t* __restrict__ prefix, int64_t n_objects, int64_t n_elems, int64_t span, Body&& body)
{
    const int64_t wg_begin = (int64_t)blockIdx.x * span;
    int64_t wg_end = wg_begin + span;
    if (wg_end > n_elems) wg_end = n_elems;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    int64_t oi = -1, o_end = 0;
    for (int64_t base = wg_begin + 64 * wave; base < wg_end; base += 256) {
        if (oi < 0) { oi = find_object(prefix, n_objects, base); o_end = prefix[oi + 1]; }
        else while (base >= o_end) { ++oi; o_end = prefix[oi + 1]; }
        const int64_t el = base + lane;
        if (base + 64 <= o_end) {
            if (el < wg_end) body(el, oi);
        } else if (el < wg_end) {
            body(el, el < o_end ? oi : find_object(prefix, n_objects, el));
        }
    }
}

// 1 / (nfft * nfft) as ims_fft_inverse's scaling pass forms it on the host (powers of two: the exponent written directly)
__device__ __forceinline__ double inv_n2(int nfft)
{
    const uint32_t n = (uint32_t)nfft;
    if ((n & (n - 1u)) == 0u) return __longlong_as_double((long long)(1023 - 2 * (31 - __clz((int)n))) << 52);
    return 1.0 / ((double)nfft * (double)nfft);
}
// a value of the real-space buffer as the image holds it (ims_fft_params_t.rbuf_raw)
__device__ __forceinline__ double rbuf_value(const double* __restrict__ rbuf, int64_t at, bool raw, double scale)
{
    const double v = rbuf[at];
    return raw ? v * scale : v;
}

// LDS tables of the pixel response for a workgroup whose span lies inside ONE object's half spectrum (every workgroup of a grid of
// 1 024 or more): sinc along x for every column of the row, sinc along y (for ky and for -ky) for the few rows the span covers.
constexpr int FILL_NH_MAX = 2049, FILL_ROWS_MAX = 264;      // grids up to 4096 (larger ones: no tables); 20 KB of LDS
// The same workgroup on a box (IMS_PROF_BOX): qx / 2 = A j + B i' and qy / 2 = C j + D i' are affine in the grid indices, so their sines
// come from {sin, cos} of (A j, C j) per column and of (B i', D i') per row by angle addition.  The columns are split in two levels,
// j = 64 jh + jl (64 + 5 entries; one level and the rows would pass the 32 KB a workgroup may hold with five on a CU), the rows are
// stored for +i' only (the mirrored row changes the sign of the sines).  10.7 KB more: 31.3 KB per workgroup.
// Grids up to BOX_NFFT_MAX only.  The parts A jl, A 64 jh and B i' are rounded one by one, so where they cancel the sum misses the
// h the plain form takes by some ulps of the PARTS, and sin / h by that over h: it grows with trail length x grid size (against the
// numpy restatement of the tests, per unit flux: 2e-16 for 12" on 256, 3e-16 to 2e-15 for 30" on 512, 3e-14 to 6e-14 for 150" on 2048
// and 8e-14 to 1e-13 for 400" on 4096 in a host emulation of this arithmetic behind Gaussians of sigma 0.4" to 0.3" -- the plain
// form rounds h as numpy does and stays at 1.4e-15).
// Neither is nearer to the exact spectrum, but larger grids keep the plain form and the bound the tests hold.
constexpr int BOX_LO = 64, BOX_NFFT_MAX = 512, BOX_HI_MAX = (BOX_NFFT_MAX / 2 + 1 + BOX_LO - 1) / BOX_LO;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_fft_kspace_fill(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                         int64_t n_objects, const int64_t* __restrict__ prefix, int64_t n_elems, int64_t span,
                                                         double* __restrict__ kbuf)
{
    __shared__ double sinc_x[FILL_NH_MAX];
    __shared__ double sinc_y[2 * FILL_ROWS_MAX];
    __shared__ double box_col[4 * (BOX_LO + BOX_HI_MAX)];
    __shared__ double box_row[4 * FILL_ROWS_MAX];
    // (uniform over the workgroup: formed from the block's number and scalar loads)
    const int64_t wg_begin = (int64_t)blockIdx.x * span;
    int64_t wg_end = wg_begin + span;
    if (wg_end > n_elems) wg_end = n_elems;
    bool tables = false, box_tables = false;
    int row_first = 0;
    if (P.n_alias <= 0 && wg_begin < wg_end) {
        const int64_t o0 = find_object(prefix, n_objects, wg_begin);
        const int64_t ob = prefix[o0];
        if (wg_end <= prefix[o0 + 1]) {
            const int n = objs[o0].nfft, nh = n / 2 + 1, half = n / 2;
            row_first = (int)((wg_begin - ob) / nh);
            const int row_last = (int)((wg_end - 1 - ob) / nh);
            if (row_first > half) return;              // rows written by the threads of their mirror rows
            if (nh <= FILL_NH_MAX && row_last - row_first + 1 <= FILL_ROWS_MAX) {
                const double dk = TWO_PI / ((double)n * P.pixel_scale);
                for (int j = threadIdx.x; j < nh; j += 256) sinc_x[j] = pixel_response((double)j * dk, P.pixel_scale);
                for (int r = threadIdx.x; r < 2 * (row_last - row_first + 1); r += 256) {
                    const double ky = (double)(row_first + (r >> 1)) * dk;
                    sinc_y[r] = pixel_response((r & 1) ? -ky : ky, P.pixel_scale);
                }
                tables = true;
                const ims_fft_object_t& ob0 = objs[o0];
#ifndef IMS_FILL_BOX_PLAIN                 // (-DIMS_FILL_BOX_PLAIN: the box by box_response's dsincos everywhere, to measure against)
                if (ob0.prof_ktable == IMS_PROF_BOX && n <= BOX_NFFT_MAX) {
                    const int n_hi = (nh + BOX_LO - 1) / BOX_LO;
                    for (int t = threadIdx.x; t < BOX_LO + n_hi; t += 256) {
                        const double kx = (double)(t < BOX_LO ? t : BOX_LO * (t - BOX_LO)) * dk;
                        dsincos(0.5 * (ob0.jac[0] * kx), box_col[4 * t], box_col[4 * t + 1]);
                        dsincos(0.5 * (ob0.jac[1] * kx), box_col[4 * t + 2], box_col[4 * t + 3]);
                    }
                    for (int r = threadIdx.x; r < row_last - row_first + 1; r += 256) {
                        const double ky = (double)(row_first + r) * dk;
                        dsincos(0.5 * (ob0.jac[2] * ky), box_row[4 * r], box_row[4 * r + 1]);
                        dsincos(0.5 * (ob0.jac[3] * ky), box_row[4 * r + 2], box_row[4 * r + 3]);
                    }
                    box_tables = true;
                }
#endif
                __syncthreads();
            }
        }
    }
    walk_span(prefix, n_objects, n_elems, span, [&](int64_t el, int64_t oi) {
        const ims_fft_object_t& o = objs[oi];
        const int64_t local = el - prefix[oi];
        const int nh = o.nfft / 2 + 1;
        int i, j;
        row_col(local, nh, i, j);
        double re, im;
        if (P.n_alias <= 0) {
            // rows i and n - i share most of their arithmetic (kspace_pair): the thread of row 0 < i < n / 2 writes both, the
            // threads of the rows beyond n / 2 have nothing to do (whole wavefronts of them: a row is nfft / 2 + 1 elements)
            const int n = o.nfft, half = n / 2;
            if (i > half) return;
            if (i > 0 && i < half) {
                const double dk = TWO_PI / ((double)n * P.pixel_scale);
                double re2, im2;
                if (box_tables) {
                    const double tab[3] = { sinc_x[j], sinc_y[2 * (i - row_first)], sinc_y[2 * (i - row_first) + 1] };
                    const double* lo = box_col + 4 * (j & (BOX_LO - 1));
                    const double* hi = box_col + 4 * (BOX_LO + j / BOX_LO);
                    const double* rw = box_row + 4 * (i - row_first);
                    const double box[8] = { fma(lo[0], hi[1], lo[1] * hi[0]), fma(lo[1], hi[1], -(lo[0] * hi[0])),
                                            fma(lo[2], hi[3], lo[3] * hi[2]), fma(lo[3], hi[3], -(lo[2] * hi[2])),
                                            rw[0], rw[1], rw[2], rw[3] };
                    kspace_pair(P, o, (double)j * dk, (double)i * dk, re, im, re2, im2, tab, box);
                } else if (tables) {
                    const double tab[3] = { sinc_x[j], sinc_y[2 * (i - row_first)], sinc_y[2 * (i - row_first) + 1] };
                    kspace_pair(P, o, (double)j * dk, (double)i * dk, re, im, re2, im2, tab);
                } else {
                    kspace_pair(P, o, (double)j * dk, (double)i * dk, re, im, re2, im2);
                }
                const int64_t at2 = o.k_offset + (int64_t)(n - i) * nh + j;
                kbuf[2 * (o.k_offset + local)] = re;
                kbuf[2 * (o.k_offset + local) + 1] = im;
                kbuf[2 * at2] = re2;
                kbuf[2 * at2 + 1] = im2;
                return;
            }
        }
        kspace_value(P, o, i, j, re, im);
        kbuf[2 * (o.k_offset + local)] = re;
        kbuf[2 * (o.k_offset + local) + 1] = im;
    });
}

// saturated bounding box of every object (saturated_region, imsim/diffraction_fft.py:211-227)
__global__ __launch_bounds__(256) void k_fft_bbox(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                  int64_t n_objects, const int64_t* __restrict__ prefix, int64_t n_pix, int64_t span,
                                                  const double* __restrict__ rbuf, int32_t* __restrict__ bbox)
{
    walk_span(prefix, n_objects, n_pix, span, [&](int64_t el, int64_t oi) {
        const ims_fft_object_t& o = objs[oi];
        const int64_t local = el - prefix[oi];
        int iy, ix;
        row_col(local, o.nfft, iy, ix);
        const int px = o.x0 + ix, py = o.y0 + iy;
        if (px < o.stamp_xmin || px > o.stamp_xmax || py < o.stamp_ymin || py > o.stamp_ymax) return;
        if (rbuf_value(rbuf, o.r_offset + local, P.rbuf_raw != 0, inv_n2(o.nfft)) > P.spikes.threshold) {
            atomicMin(&bbox[4 * oi + 0], iy); atomicMax(&bbox[4 * oi + 1], iy);
            atomicMin(&bbox[4 * oi + 2], ix); atomicMax(&bbox[4 * oi + 3], ix);
        }
    });
}

// ims_spikes_t.tab_*: one thread per row a of the stencil; b from +cutoff down to -cutoff.  row_ptr == NULL: count only.
__global__ __launch_bounds__(64) void k_fft_spike_table(const ims_spikes_t k, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ row_count,
                                                        int32_t* __restrict__ col, double* __restrict__ val)
{
    const int row = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (row > 2 * k.cutoff) return;
    const int a = row - k.cutoff;
    int n = 0;
    const int base = row_ptr ? row_ptr[row] : 0;
    for (int b = k.cutoff; b >= -k.cutoff; --b) {
        const double sv = spike_stencil(k, a, b);
        if (sv == 0.0) continue;
        if (row_ptr) { col[base + n] = b; val[base + n] = sv / k.norm; }
        ++n;
    }
    if (!row_ptr) row_count[row] = n;
}

// convolve_region (imsim/diffraction_fft.py:170-208): clipped image with the box zeroed + box (x) stencil
// Far from the arms of EVERY source pixel's cross the whole spike sum of a pixel is exact zeros: the offsets from the pixel to the
// sources differ from the offset to the box centre by at most half the box, so if even the nearer arm of the centre's cross is
// further away than that (plus the stencil's own margins, ims_fft.h spike_stencil), no term can be non-zero.  97 % of a 4096^2 stamp.
__device__ __forceinline__ bool spike_sum_is_zero(const ims_spikes_t& k, int iy, int ix, int r0, int r1, int c0, int c1)
{
    const double ac = (double)iy - 0.5 * (double)(r0 + r1), bc = (double)ix - 0.5 * (double)(c0 + c1);
    const double ha = 0.5 * (double)(r1 - r0), hb = 0.5 * (double)(c1 - c0);
    const double e = fabs(k.cos0) * ha + fabs(k.sin0) * hb + fabs(k.sin0) * ha + fabs(k.cos0) * hb;
    const double xc = k.cos0 * ac + k.sin0 * bc, yc = -k.sin0 * ac + k.cos0 * bc;
    const double mc = (fabs(xc) < fabs(yc) ? fabs(xc) : fabs(yc)) - e;
    const double rmax = sqrt(ac * ac + bc * bc) + sqrt(ha * ha + hb * hb) + 1.0;
    const double lim = 0.5 * fabs(k.d_alpha) + 1.0e-6;
    return mc > 1.0 + 1.0e-3 && mc - 1.0e-3 > lim * rmax;
}

// the spike sum of pixel (iy, ix) of object o over the saturated box rows r0 .. r1, columns c0 .. c1 (DiffractionFFT.apply's convolution)
__device__ __forceinline__ double spike_sum(const ims_fft_params_t& P, const ims_fft_object_t& o, int iy, int ix, int r0, int r1, int c0,
                                            int c1, const double* __restrict__ rin, bool raw, double scale)
{
    double acc = 0.0;
    if (P.spikes.tab_row != nullptr) {
        // The stencil's non-zero entries come out of the visit's table (ims_spikes_t.tab_*): of source row ry the entries of
        // stencil row a = iy - ry whose column offset b puts the source column ix - b inside the box, in ascending source
        // column -- the terms the loops below find among their candidates, in the same order, each formed by the same
        // operations (stencil / norm in the table's kernel, times the source here), without the three arctangents per term
        // and the ~16 candidates per row: the same sum.  (A star's spike stencil was 1.1 ms of a CCD's front, round 6.)
        // The walk is a chain of dependent loads (row pointer -> column offsets -> source pixels) on a few lanes of a wavefront, so
        // the loads are asked for in batches: the NEXT row's pointer while this row is worked on (rows are consecutive in the
        // table: row a - 1 ends where row a begins), four entries' offsets and values at once, then their four source pixels, then
        // the four terms in the table's order -- the entries with blo <= b <= bhi, a contiguous run of the descending columns, as before.
        const ims_spikes_t& k = P.spikes;
        const int blo = ix - c1, bhi = ix - c0;
        const int ry_lo = r0 > iy - k.cutoff ? r0 : iy - k.cutoff, ry_hi = r1 < iy + k.cutoff ? r1 : iy + k.cutoff;
        if (ry_lo <= ry_hi) {
            int a = iy - ry_lo;
            int e0 = k.tab_row[a + k.cutoff], e1 = k.tab_row[a + k.cutoff + 1];
            for (int ry = ry_lo; ry <= ry_hi; ++ry, --a) {
                const int e_next = ry < ry_hi ? k.tab_row[a - 1 + k.cutoff] : 0;
                int e = e0;
                if (e1 - e > 16) {                         // an arm along this row: the first entry with b <= bhi by bisection
                    int lo = e, hi = e1;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (k.tab_col[mid] > bhi) lo = mid + 1; else hi = mid; }
                    e = lo;
                }
                const int64_t row_at = o.r_offset + (int64_t)ry * o.nfft + ix;
                for (; e < e1; e += 4) {
                    int b[4];
                    double tv[4], sv[4];
                    bool use[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int eq = e + q < e1 ? e + q : e1 - 1;
                        b[q] = k.tab_col[eq]; tv[q] = k.tab_val[eq];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        use[q] = e + q < e1 && b[q] <= bhi && b[q] >= blo;
                        sv[q] = rbuf_value(rin, row_at - (use[q] ? b[q] : bhi), raw, scale);      // (not used: the box's first column)
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (use[q]) { const double src = sv[q] < 0.0 ? 0.0 : sv[q]; acc = acc + tv[q] * src; }
                    if (b[3] < blo || b[0] < blo) break;       // descending columns: nothing further down is inside the box
                }
                e1 = e0; e0 = e_next;
            }
        }
    } else {
        // Of a source row only the columns near the two arms through this pixel can contribute (|xr| or |yr| within the
        // stencil's reach T: one interval of columns each, ims_fft.h spike_stencil); everything else in the row is an exact
        // zero.  The columns are visited in ascending order as before, so the sum is the same sum -- a saturated star's
        // box is 100 x 100 source pixels, of which a target pixel on an arm needs ~16 per row.
        const ims_spikes_t& k = P.spikes;
        const double lim = 0.5 * fabs(k.d_alpha) + 1.0e-6;
        const double bfar = fabs((double)(ix - c0)) > fabs((double)(ix - c1)) ? fabs((double)(ix - c0)) : fabs((double)(ix - c1));
        const bool has_s = fabs(k.sin0) > 1.0e-12, has_c = fabs(k.cos0) > 1.0e-12;
        const double inv_s = has_s ? 1.0 / k.sin0 : 0.0, inv_c = has_c ? 1.0 / k.cos0 : 0.0;
        for (int ry = r0; ry <= r1; ++ry) {
            const int a = iy - ry;
            if (a < -k.cutoff || a > k.cutoff) continue;
            const double da = (double)a;
            const double T = 1.0 + 1.0e-3 + lim * sqrt(da * da + bfar * bfar);
            int lo[2], hi[2];
            // |cos0 a + sin0 b| <= T
            if (has_s) {
                const double b1 = (-T - k.cos0 * da) * inv_s, b2 = (T - k.cos0 * da) * inv_s;
                const double bl = b1 < b2 ? b1 : b2, bh = b1 < b2 ? b2 : b1;
                lo[0] = (int)floor((double)ix - bh) - 1; hi[0] = (int)ceil((double)ix - bl) + 1;
            } else if (fabs(k.cos0 * da) <= T) { lo[0] = c0; hi[0] = c1; }
            else { lo[0] = 1; hi[0] = 0; }
            // |-sin0 a + cos0 b| <= T
            if (has_c) {
                const double b1 = (-T + k.sin0 * da) * inv_c, b2 = (T + k.sin0 * da) * inv_c;
                const double bl = b1 < b2 ? b1 : b2, bh = b1 < b2 ? b2 : b1;
                lo[1] = (int)floor((double)ix - bh) - 1; hi[1] = (int)ceil((double)ix - bl) + 1;
            } else if (fabs(k.sin0 * da) <= T) { lo[1] = c0; hi[1] = c1; }
            else { lo[1] = 1; hi[1] = 0; }
            for (int q = 0; q < 2; ++q) { if (lo[q] < c0) lo[q] = c0; if (hi[q] > c1) hi[q] = c1; }
            if (lo[1] < lo[0]) { const int tl = lo[0], th = hi[0]; lo[0] = lo[1]; hi[0] = hi[1]; lo[1] = tl; hi[1] = th; }
            if (hi[0] >= lo[0] && hi[1] >= lo[1] && lo[1] <= hi[0] + 1) { if (hi[1] > hi[0]) hi[0] = hi[1]; lo[1] = 1; hi[1] = 0; }   // one run
            for (int q = 0; q < 2; ++q)
                for (int rx = lo[q]; rx <= hi[q]; ++rx) {
                    const int b = ix - rx;
                    if (b < -k.cutoff || b > k.cutoff) continue;
                    double src = rbuf_value(rin, o.r_offset + (int64_t)ry * o.nfft + rx, raw, scale);
                    if (src < 0.0) src = 0.0;
                    acc = acc + spike_stencil(k, a, b) / k.norm * src;
                }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_fft_spikes(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                    int64_t n_objects, const int64_t* __restrict__ prefix, int64_t n_pix, int64_t span,
                                                    const double* __restrict__ rin, double* __restrict__ rout,
                                                    const int32_t* __restrict__ bbox, const unsigned int* __restrict__ only_if_over,
                                                    unsigned int over_cap)
{
    // (the fallback of the listed form below: runs only when the list ran over)
    if (only_if_over != nullptr && only_if_over[0] <= over_cap) return;
    walk_span(prefix, n_objects, n_pix, span, [&](int64_t el, int64_t oi) {
        const ims_fft_object_t& o = objs[oi];
        const int64_t local = el - prefix[oi];
        int iy, ix;
        row_col(local, o.nfft, iy, ix);
        const bool raw = P.rbuf_raw != 0;
        const double scale = inv_n2(o.nfft);
        double v = rbuf_value(rin, o.r_offset + local, raw, scale);
        if (v < 0.0) v = 0.0;
        const int px = o.x0 + ix, py = o.y0 + iy;
        const bool in_stamp = !(px < o.stamp_xmin || px > o.stamp_xmax || py < o.stamp_ymin || py > o.stamp_ymax);
        const int r0 = bbox[4 * oi + 0], r1 = bbox[4 * oi + 1], c0 = bbox[4 * oi + 2], c1 = bbox[4 * oi + 3];
        if (P.spikes.enabled && in_stamp && r1 >= r0) {
            if (iy >= r0 && iy <= r1 && ix >= c0 && ix <= c1) v = 0.0;
            double acc = 0.0;
            if (!spike_sum_is_zero(P.spikes, iy, ix, r0, r1, c0, c1)) acc = spike_sum(P, o, iy, ix, r0, r1, c0, c1, rin, raw, scale);
            v = v + acc;
        }
        rout[o.r_offset + local] = v;
    });
}

// The spike step in two launches (ims_fft_spikes_listed).  This one streams: clip, the saturated box to zero, the image written --
// and the pixels whose spike sum is NOT known to be zero (3 % of a bright star's stamp: the arms) appended to a list, object << 40 |
// element of the object.  Light (no table walk in it: 40 registers instead of 98), so that its 16 bytes per pixel move at the
// rate of a copy; the arms' sums are then formed by k_fft_spikes_arms with every lane at work, not three in a wavefront.
__global__ __launch_bounds__(256) void k_fft_spikes_stream(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                           int64_t n_objects, const int64_t* __restrict__ prefix, int64_t n_pix, int64_t span,
                                                           const double* __restrict__ rin, double* __restrict__ rout,
                                                           const int32_t* __restrict__ bbox, unsigned long long* __restrict__ list,
                                                           unsigned int cap, unsigned int* __restrict__ count)
{
    walk_span(prefix, n_objects, n_pix, span, [&](int64_t el, int64_t oi) {
        const ims_fft_object_t& o = objs[oi];
        const int64_t local = el - prefix[oi];
        int iy, ix;
        row_col(local, o.nfft, iy, ix);
        double v = rbuf_value(rin, o.r_offset + local, P.rbuf_raw != 0, inv_n2(o.nfft));
        if (v < 0.0) v = 0.0;
        const int px = o.x0 + ix, py = o.y0 + iy;
        const bool in_stamp = !(px < o.stamp_xmin || px > o.stamp_xmax || py < o.stamp_ymin || py > o.stamp_ymax);
        const int r0 = bbox[4 * oi + 0], r1 = bbox[4 * oi + 1], c0 = bbox[4 * oi + 2], c1 = bbox[4 * oi + 3];
        bool want = false;
        if (P.spikes.enabled && in_stamp && r1 >= r0) {
            if (iy >= r0 && iy <= r1 && ix >= c0 && ix <= c1) v = 0.0;
            want = !spike_sum_is_zero(P.spikes, iy, ix, r0, r1, c0, c1);
        }
        rout[o.r_offset + local] = v;
        // one addition to the counter per wavefront
        const unsigned long long m = __ballot(want);
        if (m != 0ull) {
            const int lane = (int)(threadIdx.x & 63u), lead = __ffsll((long long)m) - 1;
            unsigned int base = 0u;
            if (lane == lead) base = atomicAdd(count, (unsigned int)__popcll(m));
            base = __shfl(base, lead, 64);
            const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
            if (want && at < cap) list[at] = ((unsigned long long)oi << 40) | (unsigned long long)local;
        }
    });
}

__global__ __launch_bounds__(256) void k_fft_spikes_arms(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                         const double* __restrict__ rin, double* __restrict__ rout,
                                                         const int32_t* __restrict__ bbox, const unsigned long long* __restrict__ list,
                                                         unsigned int cap, const unsigned int* __restrict__ count)
{
    const unsigned int n = count[0];
    if (n > cap) return;                          // the list ran over: k_fft_spikes does the whole step again
    const unsigned int stride = gridDim.x * blockDim.x;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const unsigned long long e = list[t];
        const int64_t oi = (int64_t)(e >> 40), local = (int64_t)(e & ((1ull << 40) - 1ull));
        const ims_fft_object_t& o = objs[oi];
        int iy, ix;
        row_col(local, o.nfft, iy, ix);
        const int r0 = bbox[4 * oi + 0], r1 = bbox[4 * oi + 1], c0 = bbox[4 * oi + 2], c1 = bbox[4 * oi + 3];
        const double acc = spike_sum(P, o, iy, ix, r0, r1, c0, c1, rin, P.rbuf_raw != 0, inv_n2(o.nfft));
        rout[o.r_offset + local] = rout[o.r_offset + local] + acc;
    }
}

// clip, Poisson noise, stamp -> CCD add (stamp.py:519-524); realized flux = noise-free sum inside the stamp
__global__ __launch_bounds__(256) void k_fft_finish(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                    int64_t n_objects, const int64_t* __restrict__ prefix, int64_t n_pix, int64_t span,
                                                    const double* __restrict__ rbuf)
{
    walk_span(prefix, n_objects, n_pix, span, [&](int64_t el, int64_t oi) {
        const ims_fft_object_t& o = objs[oi];
        const int64_t local = el - prefix[oi];
        int iy, ix;
        row_col(local, o.nfft, iy, ix);
        const int px = o.x0 + ix, py = o.y0 + iy;
        if (px < o.stamp_xmin || px > o.stamp_xmax || py < o.stamp_ymin || py > o.stamp_ymax) return;
        double v = rbuf_value(rbuf, o.r_offset + local, P.rbuf_raw != 0, inv_n2(o.nfft));
        if (v < 0.0) v = 0.0;
        if (P.realized_flux != nullptr && v != 0.0) unsafeAtomicAdd(P.realized_flux + oi, v);
        if (P.add_noise) v = poisson(v, P.seed, o.obj_id, local);
        const int cxp = px - P.xmin, cyp = py - P.ymin;
        if (cxp < 0 || cxp >= P.nx || cyp < 0 || cyp >= P.ny || v == 0.0) return;
        unsafeAtomicAdd(P.image + ((int64_t)cyp * P.nx + cxp), v);
    });
}

// ---- the inverse transforms of the FFT branch (hipFFT, plans cached) ----
__global__ __launch_bounds__(256) void k_scale(double* __restrict__ v, int64_t n, double s)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) v[i] = v[i] * s;
}

extern "C" {

static int fft_err(hipfftResult r, const char* what)
{
    if (r == HIPFFT_SUCCESS) return IMS_OK;
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: hipfft error %d", what, (int)r);
    return set_err(IMS_ERR_HIP, buf);
}

// Plans are kept per (size, stream) and transform ONE stamp: a batch is a loop over it.  The FIRST plan of a process costs seconds
// (measured in round 5 on a fresh box: 2.4 s for the first call -- hipFFT / rocFFT start up and compile their kernels at run time
// --, 0.5 s for the next new size, nothing after that; with a plan per size AND batch count every new combination paid again: 2.8
// of the 3.4 s a fresh process spent on its first 48 CCDs), a CCD holds one to three FFT-drawn objects of a handful of sizes, and
// a transform of 1024^2 or more fills the device by itself, so nothing is lost by not batching.  Per STREAM because a plan owns
// its work buffer (the transposes of the large sizes go through it): the same plan executing on two streams at once -- the FFT
// objects of two CCDs of a focal plane on the two top-chain streams -- would share it.  Small transforms (below 1024^2:
// launch-bound) keep batched plans.  ims_fft_warm makes the plans ahead of time (from another host thread, while the host
// still reads catalogs).

// the plan of (nfft, per_plan, stream): looked up under the lock, MADE outside it (seconds for a size's first plan: plans of
// different sizes are made side by side by ims_fft_warm's callers), entered under the lock again
static int fft_plan_get(const ims_libs::Fft* F, int32_t nfft, int64_t per_plan, void* stream, hipfftHandle* out)
{
    const std::tuple<int32_t, int64_t, void*> key(nfft, per_plan, stream);
    {
        std::lock_guard<std::mutex> lock(g_fft_mutex);
        auto it = g_fft_plans.find(key);
        if (it != g_fft_plans.end()) { *out = it->second; return IMS_OK; }
    }
    int n[2] = { nfft, nfft };
    int inembed[2] = { nfft, nfft / 2 + 1 }, onembed[2] = { nfft, nfft };
    hipfftHandle p;
    int rc = fft_err(F->plan_many(&p, 2, n, inembed, 1, nfft * (nfft / 2 + 1), onembed, 1, nfft * nfft, HIPFFT_Z2D, (int)per_plan),
                     "hipfftPlanMany");
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_fft_mutex);
    auto ins = g_fft_plans.emplace(key, p);
    if (!ins.second) (void)F->destroy(p);            // another thread was faster
    *out = ins.first->second;
    return IMS_OK;
}

int ims_fft_warm(int32_t nfft, void* stream)
{
    if (nfft < 2 || (nfft & 1)) return set_err(IMS_ERR_ARG, "nfft must be even and >= 2");
    const ims_libs::Fft* F = ims_libs::fft();
    if (!F) return set_err(IMS_ERR_UNSUPPORTED, "hipFFT is not loadable (libhipfft.so; IMS_HIPFFT_LIB names a file)");
    hipfftHandle plan;
    return fft_plan_get(F, nfft, 1, stream, &plan);
}

static int fft_inverse_impl(double* kbuf_dev, double* rbuf_dev, int32_t nfft, int64_t batch, void* stream, bool normalise)
{
    if (batch <= 0) return IMS_OK;
    if (!kbuf_dev || !rbuf_dev) return set_err(IMS_ERR_ARG, "NULL buffer");
    if (nfft < 2 || (nfft & 1) || batch > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "nfft must be even and >= 2");
    const ims_libs::Fft* F = ims_libs::fft();
    if (!F) return set_err(IMS_ERR_UNSUPPORTED, "hipFFT is not loadable (libhipfft.so; IMS_HIPFFT_LIB names a file)");
    int64_t per_plan = nfft >= 1024 ? 1 : batch;
    {
        if (per_plan != batch) {
            // a (size, batch) pair that comes again -- a replayed step, the same counts on many CCDs -- gets its batched plan (a few
            // milliseconds once the size's kernels exist: only a size's FIRST plan is expensive)
            static std::map<std::tuple<int32_t, int64_t, void*>, int> asked;
            std::lock_guard<std::mutex> lock(g_fft_mutex);
            if (++asked[std::make_tuple(nfft, batch, stream)] >= 2) per_plan = batch;
        }
        hipfftHandle plan;
        int rc = fft_plan_get(F, nfft, per_plan, stream, &plan);
        if (rc) return rc;
        // (set-stream + execute of one plan must not interleave between host threads: a plan carries its stream)
        static std::mutex exec_mutex;
        std::lock_guard<std::mutex> lock(exec_mutex);
        rc = fft_err(F->set_stream(plan, (hipStream_t)stream), "hipfftSetStream");
        if (rc) return rc;
        for (int64_t b = 0; b < batch; b += per_plan) {
            rc = fft_err(F->exec_z2d(plan, (hipfftDoubleComplex*)kbuf_dev + b * (int64_t)nfft * (nfft / 2 + 1),
                                     (hipfftDoubleReal*)rbuf_dev + b * (int64_t)nfft * nfft), "hipfftExecZ2D");
            if (rc) return rc;
        }
    }
    if (!normalise) return IMS_OK;          // the readers multiply (ims_fft_params_t.rbuf_raw)
    // numpy / GalSim normalisation of the inverse ("backward": 1 / N^2): exact for the even sizes used (powers of two)
    const int64_t total = batch * (int64_t)nfft * nfft;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_scale, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rbuf_dev, total, 1.0 / ((double)nfft * (double)nfft));
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_fft_inverse(double* kbuf_dev, double* rbuf_dev, int32_t nfft, int64_t batch, void* stream)
{
    return fft_inverse_impl(kbuf_dev, rbuf_dev, nfft, batch, stream, true);
}

int ims_fft_inverse_raw(double* kbuf_dev, double* rbuf_dev, int32_t nfft, int64_t batch, void* stream)
{
    return fft_inverse_impl(kbuf_dev, rbuf_dev, nfft, batch, stream, false);
}

// a workgroup's share of the elements of an elementwise FFT kernel (walk_span): at least 4 096 workgroups where the elements allow it
// (256 CUs x 16), at most 8 192 elements each (32 passes per lookup of the object; short enough that a star's core rows, where a
// pixel costs many times a pixel of the wings, spread over many workgroups)
struct FftSpan { int64_t span; unsigned grid; };
static FftSpan fft_span(int64_t n)
{
    int64_t span = ((n + 4095) / 4096 + 255) / 256 * 256;
    if (span < 256) span = 256;
    if (span > 8192) span = 8192;
    return { span, (unsigned)((n + span - 1) / span) };
}

int ims_fft_kspace_fill(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, int64_t n_objects,
                        const int64_t* elem_prefix_dev, int64_t n_elems, double* kbuf, void* stream)
{
    if (!params || !objects_dev || !elem_prefix_dev || !kbuf) return set_err(IMS_ERR_ARG, "NULL argument");
    if (params->n_kpsf < 0 || params->n_kpsf > IMS_MAX_PSF) return set_err(IMS_ERR_ARG, "n_kpsf out of range");
    if (n_objects <= 0 || n_elems <= 0) return IMS_OK;
    {
        LaunchTimer tm((hipStream_t)stream, 3);
        const FftSpan sp = fft_span(n_elems);
        hipLaunchKernelGGL(k_fft_kspace_fill, dim3(sp.grid), dim3(256), 0, (hipStream_t)stream, *params, objects_dev,
                           n_objects, elem_prefix_dev, n_elems, sp.span, kbuf);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

__global__ void k_fill_bbox(int32_t* bbox, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { bbox[4 * i + 0] = 0x7fffffff; bbox[4 * i + 1] = -1; bbox[4 * i + 2] = 0x7fffffff; bbox[4 * i + 3] = -1; }
}

int ims_fft_spike_table(const ims_spikes_t* spikes, const int32_t* row_ptr_dev, int32_t* row_count_dev, int32_t* col_dev, double* val_dev,
                        void* stream)
{
    if (!spikes) return set_err(IMS_ERR_ARG, "spikes is NULL");
    if (spikes->cutoff < 0 || spikes->cutoff > 32767 || !(spikes->norm > 0.0)) return set_err(IMS_ERR_ARG, "spikes: cutoff / norm out of range");
    if (row_ptr_dev ? (!col_dev || !val_dev) : !row_count_dev) return set_err(IMS_ERR_ARG, "spike table: NULL output");
    ims_spikes_t k = *spikes;
    k.tab_row = nullptr; k.tab_col = nullptr; k.tab_val = nullptr;
    const unsigned rows = 2u * (unsigned)k.cutoff + 1u;
    hipLaunchKernelGGL(k_fft_spike_table, dim3((rows + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, k, row_ptr_dev, row_count_dev, col_dev, val_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_fft_spikes(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, int64_t n_objects,
                   const int64_t* pix_prefix_dev, int64_t n_pix, const double* rbuf_in, double* rbuf_out,
                   int32_t* bbox_dev, void* stream)
{
    if (!params || !objects_dev || !pix_prefix_dev || !rbuf_in || !rbuf_out || !bbox_dev) return set_err(IMS_ERR_ARG, "NULL argument");
    if (n_objects <= 0 || n_pix <= 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fill_bbox, dim3((unsigned)((n_objects + 255) / 256)), dim3(256), 0, st, bbox_dev, n_objects);
    const FftSpan sp = fft_span(n_pix);
    if (params->spikes.enabled)
        hipLaunchKernelGGL(k_fft_bbox, dim3(sp.grid), dim3(256), 0, st, *params, objects_dev, n_objects,
                           pix_prefix_dev, n_pix, sp.span, rbuf_in, bbox_dev);
    hipLaunchKernelGGL(k_fft_spikes, dim3(sp.grid), dim3(256), 0, st, *params, objects_dev, n_objects,
                       pix_prefix_dev, n_pix, sp.span, rbuf_in, rbuf_out, (const int32_t*)bbox_dev, (const unsigned int*)nullptr, 0u);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_fft_spikes_listed(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, int64_t n_objects,
                          const int64_t* pix_prefix_dev, int64_t n_pix, const double* rbuf_in, double* rbuf_out,
                          int32_t* bbox_dev, uint64_t* list_dev, int64_t list_cap, uint32_t* count_dev, void* stream)
{
    if (!params || !objects_dev || !pix_prefix_dev || !rbuf_in || !rbuf_out || !bbox_dev || !list_dev || !count_dev)
        return set_err(IMS_ERR_ARG, "NULL argument");
    if (list_cap < 1 || list_cap > 0xffffffffLL) return set_err(IMS_ERR_ARG, "list_cap out of range");
    if (n_objects >= (1ll << 24)) return set_err(IMS_ERR_ARG, "the listed spike step holds at most 2^24 objects");
    if (n_objects <= 0 || n_pix <= 0) return IMS_OK;
    if (!params->spikes.enabled) return ims_fft_spikes(params, objects_dev, n_objects, pix_prefix_dev, n_pix, rbuf_in, rbuf_out, bbox_dev, stream);
    hipStream_t st = (hipStream_t)stream;
    const unsigned int cap = (unsigned int)list_cap;
    HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_fill_bbox, dim3((unsigned)((n_objects + 255) / 256)), dim3(256), 0, st, bbox_dev, n_objects);
    const FftSpan sp = fft_span(n_pix);
    hipLaunchKernelGGL(k_fft_bbox, dim3(sp.grid), dim3(256), 0, st, *params, objects_dev, n_objects,
                       pix_prefix_dev, n_pix, sp.span, rbuf_in, bbox_dev);
    hipLaunchKernelGGL(k_fft_spikes_stream, dim3(sp.grid), dim3(256), 0, st, *params, objects_dev, n_objects, pix_prefix_dev, n_pix,
                       sp.span, rbuf_in, rbuf_out, (const int32_t*)bbox_dev, (unsigned long long*)list_dev, cap, (unsigned int*)count_dev);
    // the arms: a grid that covers the list at 256 entries per workgroup, at most 16 384 workgroups (they stride)
    int64_t arms = (list_cap + 255) / 256;
    if (arms > 16384) arms = 16384;
    hipLaunchKernelGGL(k_fft_spikes_arms, dim3((unsigned)arms), dim3(256), 0, st, *params, objects_dev, rbuf_in, rbuf_out,
                       (const int32_t*)bbox_dev, (const unsigned long long*)list_dev, cap, (const unsigned int*)count_dev);
    // more arm pixels than the list holds: the whole step once more in one launch (returns at once otherwise)
    hipLaunchKernelGGL(k_fft_spikes, dim3(sp.grid), dim3(256), 0, st, *params, objects_dev, n_objects, pix_prefix_dev, n_pix, sp.span,
                       rbuf_in, rbuf_out, (const int32_t*)bbox_dev, (const unsigned int*)count_dev, cap);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_fft_finish(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, int64_t n_objects,
                   const int64_t* pix_prefix_dev, int64_t n_pix, const double* rbuf, void* stream)
{
    if (!params || !objects_dev || !pix_prefix_dev || !rbuf) return set_err(IMS_ERR_ARG, "NULL argument");
    if (!params->image) return set_err(IMS_ERR_ARG, "image is NULL");
    if (n_objects <= 0 || n_pix <= 0) return IMS_OK;
    const FftSpan sp = fft_span(n_pix);
    hipLaunchKernelGGL(k_fft_finish, dim3(sp.grid), dim3(256), 0, (hipStream_t)stream, *params, objects_dev,
                       n_objects, pix_prefix_dev, n_pix, sp.span, rbuf);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
