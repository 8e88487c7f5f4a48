// imsim_hip.hip -- kernels and C-ABI entry points of libimsim_hip.so (gfx950 / MI355X only).
//
// Launch geometry: one 256-thread workgroup (4 wavefronts of 64) per *segment* = up to seg_size
// photons of ONE object, so the object row, its stamp and its tables are wave-uniform (scalar
// loads) and the per-object flux reduction is a wavefront shuffle + one atomic per wave.
// Segments are dealt to the 8 XCDs in contiguous ranges (block b runs on XCD b%8 on this part),
// so that objects that are neighbours in the (spatially sorted) table share an XCD's L2 for the
// pixel-boundary state and the image lines they touch.
//
// ONE translation unit, written as sections: ims_host.h (the library's host state and the helpers every entry point uses),
// this file, then one file per subsystem (ims_image.h .. ims_test.h, included at the end).  A section holds its kernels, its
// static host helpers and its own extern "C" block, and needs only what is included before it (DESIGN.md has the file map).
// This file is the hot path alone: the photon kernels, the joint rounds, the Silicon boundary state and their entry points.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include <mutex>
#include <unordered_map>
#include <map>
#include <tuple>
#include "ims_photon.h"
#include "ims_fft.h"
#include "ims_libs.h"           // hipFFT / RCCL looked up at run time (the handle types the host state names)

using namespace ims;

#include "ims_host.h"           // host state, error / launch helpers, ims_abi_version .. ims_last_kernel_ms, ims_struct_size

// ---------------- segment -> (object, first photon) ----------------

__device__ __forceinline__ int64_t xcd_segment(int64_t b, int64_t n_segments)
{
    // block b runs on XCD (b % 8): give each XCD one contiguous range of segments
    const int64_t per = (n_segments + N_XCD - 1) / N_XCD;
    return (b % N_XCD) * per + (b / N_XCD);
}

// the last entry of an int64 prefix that is <= seg: the object of a segment here and in the PSF probes, the object of a grid
// element on the FFT branch (ims_fft_branch.h), the object and the tile of a photon in ims_reshoot.h
__device__ __forceinline__ int64_t find_object(const int64_t* __restrict__ prefix, int64_t n_objects, int64_t seg)
{
    int64_t lo = 0, hi = n_objects;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= seg) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// run one photon through shoot -> psf -> shift -> ops
template <int PSF = 0>
__device__ __forceinline__ void make_photon(const ims_render_params_t& P, const ims_object_t& o, int64_t k, Rng& rng, Photon& ph)
{
    rng_reset(rng);
    shoot(P, o, k, rng, ph);
    run_psf<PSF>(P, o, k, rng, ph);
    ph.x = o.x0 + ph.x;
    ph.y = o.y0 + ph.y;
}

// ---------------- per-workgroup charge tile ----------------
// All photons of a workgroup belong to ONE object, and a bright star puts thousands of photons per
// round into a few dozen pixels: global atomics on those hot addresses serialise in L2.  Each
// workgroup therefore first sums its photons into a 32x32-pixel LDS tile centred on the object
// (ds_add_f32), then flushes each non-empty tile cell with ONE global atomic to the CCD image (and
// to the delta-charge image when the object's region is brighter-fatter tracked).  Photons outside
// the tile go straight to global memory.  Unit fluxes keep every partial sum an exact integer, so
// the result stays independent of the order of the atomics.  A photon whose flux is not exactly 1
// (BandpassRatio reweighting, flux_per_photon != 1) never enters the float tile: it is added to the
// f64 image directly, so no rounding to binary32 happens anywhere on its way.
constexpr int CT = 32;

// Joint rounds whose update / refresh walk LISTS of tiles: the pixel search appends a tile the first time charge lands within the
// update's reach of it (k_accumulate_round_j; ims_tuning_t.joint_search_lists), instead of a launch of its own that scans the
// charge marks of every tile of every region afterwards (k_build_active_j: 13 - 32 us of every round of a joint run).
struct JointAcc;
struct JointRound;
constexpr int IMS_JOINT_MAX = 64;          // chains of one joint launch (JOINT rounds, below)
constexpr int ENTRY_CHAIN_BITS = 6, ENTRY_SLOT_BITS = 26, ENTRY_TILE_BITS = 32;     // a tile-list entry: chain << 58 | slot of the class << 32 | tile
static_assert(ENTRY_CHAIN_BITS + ENTRY_SLOT_BITS + ENTRY_TILE_BITS == 64 && IMS_JOINT_MAX <= (1 << ENTRY_CHAIN_BITS), "chain field too narrow");
__device__ __forceinline__ unsigned long long pack_tile_entry(int chain, int slot, int tile)
{
    return ((unsigned long long)chain << (64 - ENTRY_CHAIN_BITS)) | ((unsigned long long)(unsigned int)slot << ENTRY_TILE_BITS) | (unsigned int)tile;
}
__device__ __forceinline__ void unpack_tile_entry(unsigned long long e, int& chain, int& slot, int& tile)
{
    chain = (int)(e >> (64 - ENTRY_CHAIN_BITS)); slot = (int)((e >> ENTRY_TILE_BITS) & ((1u << ENTRY_SLOT_BITS) - 1u)); tile = (int)(e & 0xFFFFFFFFu);
}
struct TileLister {
    unsigned long long* list = nullptr; // entries: pack_tile_entry; NULL: no listing (the default)
    int* count = nullptr;               // entries so far (this round's parity)
    const JointAcc* J = nullptr;        // per chain: tile words, tiles before each slot of the class, the class's first slot
    const JointRound* R = nullptr;      // per chain: tiles of the regions that go on after this round (only those are updated)
    int chain = 0;
    unsigned int round_word = 0u;       // this round + 1
};
// (resolved where the lists are written, at the end of the workgroup: kept live through the pixel search, the chain's table
// entries cost the search kernel its register allocation -- 96 registers and scratch instead of 93)
struct TileListerChain { unsigned int* words; int64_t tile_base; int lo; bool on; };
__device__ __forceinline__ TileListerChain lister_chain(const TileLister& L, int slot_idx);

struct ChargeTile {
    int x0, y0;                // pixel coordinates of tile cell (0,0)
    bool track;                // also add to the slot's delta image
    ims_bf_slot_t slot;
    TileLister lister{};       // joint rounds with search-side lists (by value: through a pointer the block lived in scratch); list == NULL: off
    int slot_idx = 0;          // the region's slot
};

__device__ __forceinline__ void tile_begin(float* tile, ChargeTile& ct, const ims_render_params_t& P, const ims_object_t& o,
                                           bool silicon, int n_thr = 256, const TileLister* lister = nullptr)
{
    for (int e = threadIdx.x; e < CT * CT; e += n_thr) tile[e] = 0.0f;
    ct.x0 = (int)floor(o.x0 + 0.5) - CT / 2;
    ct.y0 = (int)floor(o.y0 + 0.5) - CT / 2;
    ct.track = silicon && !(o.flags & IMS_OBJ_FAINT) && (o.bf_state > 0 || P.track_static_delta);
    ct.lister.list = nullptr; ct.slot_idx = 0;
    if (ct.track) { ct.slot_idx = slot_index(P, o); ct.slot = P.sensor->bf_slots[ct.slot_idx]; }
    if (ct.track && lister != nullptr && lister->list != nullptr) ct.lister = *lister;
    __syncthreads();
}

// bf_tag != 0: remember which 16x16 tile of the region received charge (byte at the tile's first cell)
__device__ __forceinline__ void mark_tile_charge(const ims_render_params_t& P, int64_t offset, int nx, int di, int dj)
{
    if (P.bf_tag == 0u) return;
    unsigned char* tc = P.sensor->bf_tile_charge;
    if (tc == nullptr) return;
    tc[offset + (int64_t)(dj & ~15) * (nx + 1) + (di & ~15)] = (unsigned char)P.bf_tag;
    // and which 4 x 4 block of it: the byte of the block's cell (1, 1) -- never a tile's first cell, and inside the region's
    // (nx + 1) x (ny + 1) owner cells because (di & ~3) + 1 <= di + 1 <= nx.  Read by k_build_active_j.
    tc[offset + (int64_t)((dj & ~3) + 1) * (nx + 1) + ((di & ~3) + 1)] = (unsigned char)P.bf_tag;
}

// Charge landed on pixel (di, dj) of the region: list every tile whose update or bounds refresh can depend on it and that no
// deposit of this round has listed yet.  The update of tile [tx0, tx0 + 15]^2 reads the delta charge of [tx0 - 4, tx0 + 18]^2, the
// bounds of its pixels also hang on the first column / row of the right / upper tile, which move with charge up to tx0 + 19: the
// tiles tx with tx0 - 4 <= di <= tx0 + 19, the same in y -- one, two or four tiles.  A tile's word holds the last round that
// listed it: the exchange decides who appends (a stale plain read only costs the exchange).
__device__ __forceinline__ void list_tiles_in_reach(const ChargeTile& ct, int di, int dj)
{
    const TileLister& L = ct.lister;
    const TileListerChain C = lister_chain(L, ct.slot_idx);
    if (!C.on) return;
    const int tiles_x = (ct.slot.nx + 1 + 15) >> 4, tiles_y = (ct.slot.ny + 1 + 15) >> 4;
    int ax = (di - 4) >> 4, bx = (di + 4) >> 4, ay = (dj - 4) >> 4, by = (dj + 4) >> 4;
    if (ax < 0) ax = 0;
    if (ay < 0) ay = 0;
    if (bx > tiles_x - 1) bx = tiles_x - 1;
    if (by > tiles_y - 1) by = tiles_y - 1;
    for (int ty = ay; ty <= by; ++ty)
        for (int tx = ax; tx <= bx; ++tx) {
            const int t = ty * tiles_x + tx;
            unsigned int* w = C.words + (C.tile_base + t);
            if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == L.round_word) continue;
            if (atomicExch(w, L.round_word) == L.round_word) continue;
            const int k = atomicAdd(L.count, 1);
            L.list[k] = pack_tile_entry(L.chain, C.lo, t);
        }
}

// list_now: the deposit lists its tiles itself (the stragglers outside the workgroup's LDS tile); the flush of the LDS tile
// collects the tiles of all its deposits first (tile_flush)
__device__ __forceinline__ void deposit_global(const ims_render_params_t& P, const ChargeTile& ct, int ix, int iy, double flux,
                                               bool list_now = true)
{
    const int px = ix - P.xmin, py = iy - P.ymin;
    bool to_image = px >= 0 && px < P.nx && py >= 0 && py < P.ny;
    if (ct.track) {
        const int di = ix - ct.slot.xmin, dj = iy - ct.slot.ymin;
        if (di >= 0 && di < ct.slot.nx && dj >= 0 && dj < ct.slot.ny) {
            unsafeAtomicAdd(P.sensor->bf_delta + (ct.slot.offset + (int64_t)dj * (ct.slot.nx + 1) + di), flux);
            mark_tile_charge(P, ct.slot.offset, ct.slot.nx, di, dj);
            if (list_now && ct.lister.list != nullptr) list_tiles_in_reach(ct, di, dj);
            // track_static_delta 2 (photon pooling, slot 0 = the image): the image takes the charge FROM the delta image when
            // the recalculation consumes it -- GalSim's `target += delta` -- so the deposit is one atomic add, not two
            if (P.track_static_delta == 2) to_image = false;
        }
    }
    if (to_image) unsafeAtomicAdd(P.image + ((int64_t)py * P.nx + px), flux);
}

__device__ __forceinline__ void tile_deposit(float* tile, const ChargeTile& ct, const ims_render_params_t& P, int ix, int iy,
                                             double flux)
{
    const int tx = ix - ct.x0, ty = iy - ct.y0;
    if (flux == 1.0 && tx >= 0 && tx < CT && ty >= 0 && ty < CT) atomicAdd(&tile[ty * CT + tx], 1.0f);
    else deposit_global(P, ct, ix, iy, flux);
}

__device__ __forceinline__ void tile_flush(float* tile, const ChargeTile& ct, const ims_render_params_t& P, int n_thr = 256)
{
    // search-side lists: the deposits of the 32 x 32 LDS tile reach at most 4 x 4 tiles of the region (pixels d0 - 4 .. d0 + 35):
    // their bits are collected in LDS, then ONE lane per tile in reach asks the tile's word, and ONE atomic per workgroup makes
    // room in the list (a deposit-by-deposit form spent the round in exchanges and in additions to the one counter)
    __shared__ unsigned int reach_bits;
    __shared__ int n_new, base_new;
    __shared__ int new_tile[16];
    const bool listing = ct.lister.list != nullptr;      // uniform over the workgroup (one object, one slot)
    if (listing && threadIdx.x == 0) { reach_bits = 0u; n_new = 0; }
    __syncthreads();
    PROBE(5);
    PROBE_WG(6, 0);
    const int tiles_x = listing ? ((ct.slot.nx + 1 + 15) >> 4) : 0, tiles_y = listing ? ((ct.slot.ny + 1 + 15) >> 4) : 0;
    int ox = listing ? ((ct.x0 - ct.slot.xmin - 4) >> 4) : 0, oy = listing ? ((ct.y0 - ct.slot.ymin - 4) >> 4) : 0;
    if (ox < 0) ox = 0;
    if (oy < 0) oy = 0;
    for (int e = threadIdx.x; e < CT * CT; e += n_thr) {
        const float v = tile[e];
        if (v != 0.0f) {
            const int ix = ct.x0 + e % CT, iy = ct.y0 + e / CT;
            deposit_global(P, ct, ix, iy, (double)v, false);
            if (listing) {
                const int di = ix - ct.slot.xmin, dj = iy - ct.slot.ymin;
                if (di >= 0 && di < ct.slot.nx && dj >= 0 && dj < ct.slot.ny) {
                    // tiles ax .. bx by ay .. by, relative to the window's first tile: a 4-bit run in x times a 4-bit run in y
                    int ax = ((di - 4) >> 4) - ox, bx = ((di + 4) >> 4) - ox, ay = ((dj - 4) >> 4) - oy, by = ((dj + 4) >> 4) - oy;
                    if (ax < 0) ax = 0;
                    if (ay < 0) ay = 0;
                    const unsigned int xm = ((2u << bx) - 1u) & ~((1u << ax) - 1u) & 0xFu;
                    const unsigned int ym = ((2u << by) - 1u) & ~((1u << ay) - 1u) & 0xFu;
                    const unsigned int rows = (ym & 1u) | ((ym & 2u) << 3) | ((ym & 4u) << 6) | ((ym & 8u) << 9);
                    atomicOr(&reach_bits, xm * rows);
                }
            }
        }
    }
    if (!listing) return;
    __syncthreads();
    const TileLister& L = ct.lister;
    if (reach_bits == 0u) return;
    const TileListerChain C = lister_chain(L, ct.slot_idx);
    if (!C.on) return;
    if (threadIdx.x < 16 && ((reach_bits >> threadIdx.x) & 1u)) {
        const int tx = ox + (int)(threadIdx.x & 3), ty = oy + (int)(threadIdx.x >> 2);
        if (tx < tiles_x && ty < tiles_y) {
            const int t = ty * tiles_x + tx;
            unsigned int* w = C.words + (C.tile_base + t);
            if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != L.round_word && atomicExch(w, L.round_word) != L.round_word)
                new_tile[atomicAdd(&n_new, 1)] = t;
        }
    }
    __syncthreads();
    if (n_new > 0) {
        if (threadIdx.x == 0) base_new = atomicAdd(L.count, n_new);
        __syncthreads();
        if ((int)threadIdx.x < n_new)
            L.list[base_new + threadIdx.x] = pack_tile_entry(L.chain, C.lo, new_tile[threadIdx.x]);
    }
}

// ---------------- fused kernel: LSST_Silicon draw (phot) + stamp->CCD add ----------------
#ifndef IMS_FUSED_WAVES
#define IMS_FUSED_WAVES 4
#endif
#ifndef IMS_CHAIN_WAVES
#define IMS_CHAIN_WAVES 4          // wavefronts per SIMD the kernels specialised for the default chain are compiled for
#endif
template <int CHAIN, int PSF = 0, unsigned long long LAYOUT = 0ull>
__global__ __launch_bounds__(256, (CHAIN == 1) ? IMS_CHAIN_WAVES : IMS_FUSED_WAVES) void k_shoot_accumulate(const ims_render_params_t P)
{
    const int64_t per = (P.n_segments + N_XCD - 1) / N_XCD;
    const int64_t b = blockIdx.x;
    if ((b / N_XCD) >= per) return;
    const int64_t seg = xcd_segment(b, P.n_segments);
    if (seg >= P.n_segments) return;
    const int64_t oi = P.seg_object ? (int64_t)P.seg_object[seg] : find_object(P.seg_prefix, P.n_objects, seg);
    const ims_object_t& o = P.objects[oi];
    const int64_t seg_in_obj = seg - P.seg_prefix[oi];
    const int64_t j0 = seg_in_obj * P.seg_size;
    int64_t j1 = j0 + P.seg_size;
    if (j1 > o.n_phot) j1 = o.n_phot;
    // Wavefronts of the workgroup that hold no photon of this segment (a 19-photon object uses one of four) leave at
    // once: they would only sit in the barriers and keep the wave slots other segments could run in.  The hardware
    // barrier counts the waves that are still alive.
    if constexpr (PSF >= 3) optical_setup(P, o);     // the object's optical phase screen, by all 256 threads (ims_optical.h)
    const int n_thr = (((int)(j1 - j0) + 63) >> 6) << 6;
    if ((int)threadIdx.x >= n_thr) return;
    const bool silicon = (P.sensor != nullptr) && (P.sensor->kind == IMS_SENSOR_SILICON);
    const bool has_angles = (CHAIN == 1) ? true : chain_has_angles(P);
    __shared__ float tile[CT * CT];
    ChargeTile ct;
    tile_begin(tile, ct, P, o, silicon, n_thr);
    double added = 0.0;
    // exactly one photon per thread (seg_size == workgroup size): no photon loop, so the compiler
    // cannot hoist the chain's uniform operands across iterations into registers
    const int64_t j = j0 + threadIdx.x;
    if (j < j1) {
        const int64_t k = o.phot_first + j;
        Photon ph;
        Rng rng;
        make_photon<PSF>(P, o, k, rng, ph);
        run_ops<CHAIN, LAYOUT>(P, o, k, rng, ph);
        int ix, iy;
        if (ph.flux != 0.0 && land(P, o, k, rng, ph, silicon, has_angles, ix, iy, seg * 4 + (int64_t)(threadIdx.x >> 6))) {
            added += ph.flux;
            tile_deposit(tile, ct, P, ix, iy, ph.flux);
        }
    }
    tile_flush(tile, ct, P, n_thr);
    if (P.realized_flux != nullptr) {
        const double tot = wave_sum(added);
        if ((threadIdx.x & 63) == 0 && tot != 0.0) unsafeAtomicAdd(P.realized_flux + oi, tot);
    }
}

// ---------------- pooled path ----------------
// LSST_PhotonsBuilder.draw for all objects of a sub-batch, written straight into the merged pool.
// MODE 1 additionally runs the configured photon-op chain before storing (used to pre-compute the
// sensor-independent part of bright objects' photons, see Renderer.plan_lsst_image); MODE 2 also runs the half of
// SiliconSensor.accumulate that does not depend on the pixel boundaries and stores the `converted` pool format
// (ims_photons_t.converted), so that the latency-bound rounds of a brighter-fatter chain only do the pixel search.
// pool.pupil_u / pupil_v / time / obj_index may be NULL (not stored).
template <int MODE, int CHAIN = 0, int PSF = 0, unsigned long long LAYOUT = 0ull>
__global__ __launch_bounds__(256, (CHAIN == 1) ? IMS_CHAIN_WAVES : IMS_FUSED_WAVES) void k_shoot_photons(const ims_render_params_t P,
                                                                        const int64_t* __restrict__ photon_offset,
                                                                        const ims_photons_t pool)
{
    const int64_t per = (P.n_segments + N_XCD - 1) / N_XCD;
    const int64_t b = blockIdx.x;
    if ((b / N_XCD) >= per) return;
    const int64_t seg = xcd_segment(b, P.n_segments);
    if (seg >= P.n_segments) return;
    const int64_t oi = P.seg_object ? (int64_t)P.seg_object[seg] : find_object(P.seg_prefix, P.n_objects, seg);
    const ims_object_t& o = P.objects[oi];
    if constexpr (PSF >= 3) optical_setup(P, o);     // the object's optical phase screen, by all 256 threads (ims_optical.h)
    const int64_t j = (seg - P.seg_prefix[oi]) * P.seg_size + threadIdx.x;
    if (j >= o.n_phot) return;
    const int64_t k = o.phot_first + j;
    Photon ph;
    Rng rng;
    make_photon<PSF>(P, o, k, rng, ph);
    if (MODE >= 1) run_ops<CHAIN, LAYOUT>(P, o, k, rng, ph);
    const int64_t i = photon_offset[oi] + j;
    if (MODE == 2) {
        const bool silicon = (P.sensor != nullptr) && (P.sensor->kind == IMS_SENSOR_SILICON);
        double x0 = ph.x, y0 = ph.y, flux = ph.flux, zs = 1.0;
        if (silicon && !(o.flags & IMS_OBJ_FAINT) && flux != 0.0) {
            double zconv;
            bool coin;
            if (land_convert(P, o, k, rng, ph, (CHAIN == 1) ? true : chain_has_angles(P), x0, y0, zconv, coin)) {
                const double zf = dtanh_pos(ddiv(zconv, 12.0));
                zs = coin ? -zf : zf;
            } else flux = 0.0;
        }
        pool.x[i] = x0; pool.y[i] = y0; pool.flux[i] = flux; pool.dxdz[i] = zs;
        return;
    }
    pool.x[i] = ph.x; pool.y[i] = ph.y; pool.flux[i] = ph.flux;
    pool.dxdz[i] = ph.dxdz; pool.dydz[i] = ph.dydz; pool.wavelength[i] = ph.wl;
    if (pool.pupil_u) { pool.pupil_u[i] = ph.pu; pool.pupil_v[i] = ph.pv; pool.time[i] = ph.t; }
    if (pool.obj_index) pool.obj_index[i] = (int32_t)oi;
}

// ---------------- PSF moments: the photons reduced instead of landed (ims_psf_moments) ----------------
// The rows are field points.  Photon k of a row is the photon k_shoot_photons makes for it -- the same device functions on the same
// Philox counters -- but nothing of it is stored: its weight and its offset from the row's nominal position go into six f64 sums
// and two counts.  stage 1: after shoot + run_psf, the offset as the PSF kicks leave it (the units of the row's winv; x0, y0 not
// added).  stage 2: after run_ops as well, position minus (x0, y0).  A photon whose flux is zero (vignetted, or its ray failed)
// is counted as dropped and adds exact zeros.
// Every sum is formed in a fixed order: the xor butterfly over the 64 lanes of a wavefront, the four wavefronts of the workgroup
// in turn through LDS, one record per 256-photon segment; then one workgroup per row adds the row's records -- thread t those of
// the segments t, t + 256, ... in turn, then the same two steps.  No atomics: a row's result depends on nothing but the row.
constexpr int PM_N = 8;            // sum w, w x, w y, w x^2, w x y, w y^2, photons used, photons dropped (counts as exact f64 integers)

// the workgroup's totals: thread q < PM_N returns total q, the others 0
__device__ __forceinline__ double moments_block_sum(double (&v)[PM_N])
{
    __shared__ double part[4][PM_N];
#pragma unroll
    for (int q = 0; q < PM_N; ++q) v[q] = wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < PM_N; ++q) part[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    const int q = (int)threadIdx.x;
    return q < PM_N ? ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q] : 0.0;
}

template <int CHAIN, int PSF, unsigned long long LAYOUT>
__global__ __launch_bounds__(256, IMS_FUSED_WAVES) void k_psf_moments(const ims_render_params_t P, const int stage,
                                                                      double* __restrict__ partial)
{
    const int64_t per = (P.n_segments + N_XCD - 1) / N_XCD;
    const int64_t b = blockIdx.x;
    if ((b / N_XCD) >= per) return;
    const int64_t seg = xcd_segment(b, P.n_segments);
    if (seg >= P.n_segments) return;
    const int64_t oi = P.seg_object ? (int64_t)P.seg_object[seg] : find_object(P.seg_prefix, P.n_objects, seg);
    const ims_object_t& o = P.objects[oi];
    if constexpr (PSF >= 3) optical_setup(P, o);     // the row's optical phase screen, by all 256 threads (ims_optical.h)
    const int64_t j = (seg - P.seg_prefix[oi]) * P.seg_size + threadIdx.x;
    double v[PM_N] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    // (the lanes past the row's last photon stay: they hold the zeros of the sums)
    if (j < o.n_phot) {
        const int64_t k = o.phot_first + j;
        Photon ph;
        Rng rng;
        rng_reset(rng);
        shoot(P, o, k, rng, ph);
        run_psf<PSF>(P, o, k, rng, ph);
        double dx = ph.x, dy = ph.y;
        if (stage == 2) {
            ph.x = o.x0 + ph.x;
            ph.y = o.y0 + ph.y;
            run_ops<CHAIN, LAYOUT>(P, o, k, rng, ph);
            dx = ph.x - o.x0; dy = ph.y - o.y0;
        }
        if (ph.flux != 0.0) {
            const double w = ph.flux, wx = w * dx, wy = w * dy;
            v[0] = w; v[1] = wx; v[2] = wy; v[3] = wx * dx; v[4] = wx * dy; v[5] = wy * dy; v[6] = 1.0;
        } else v[7] = 1.0;
    }
    const double tot = moments_block_sum(v);
    if (threadIdx.x < PM_N) partial[seg * PM_N + threadIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_psf_moments_combine(const int64_t* __restrict__ seg_prefix, const double* __restrict__ partial,
                                                             double* __restrict__ sums, int64_t* __restrict__ counts)
{
    const int64_t oi = blockIdx.x;
    const int64_t s0 = seg_prefix[oi], s1 = seg_prefix[oi + 1];
    double v[PM_N] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int64_t s = s0 + threadIdx.x; s < s1; s += 256) {
#pragma unroll
        for (int q = 0; q < PM_N; ++q) v[q] = v[q] + partial[s * PM_N + q];
    }
    const double tot = moments_block_sum(v);
    if (threadIdx.x < 6) sums[oi * 6 + threadIdx.x] = tot;
    else if (threadIdx.x < PM_N) counts[oi * 2 + (threadIdx.x - 6)] = (int64_t)tot;
}

__device__ __forceinline__ void load_photon(const ims_photons_t& pool, int64_t i, Photon& ph)
{
    ph.x = pool.x[i]; ph.y = pool.y[i]; ph.flux = pool.flux[i]; ph.dxdz = pool.dxdz[i]; ph.dydz = pool.dydz[i];
    ph.wl = pool.wavelength[i]; ph.pu = pool.pupil_u[i]; ph.pv = pool.pupil_v[i]; ph.t = pool.time[i];
}

// `for op in photon_ops: op.applyTo(photons, ...)` (photon_pooling.py:154-155): one pass, all ops
template <unsigned long long LAYOUT = 0ull>
__global__ __launch_bounds__(256) void k_apply_ops(const ims_render_params_t P, const int64_t* __restrict__ photon_offset,
                                                   const ims_photons_t pool)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pool.n; i += stride) {
        const int32_t oi = pool.obj_index[i];
        const ims_object_t& o = P.objects[oi];
        const int64_t k = o.phot_first + (i - photon_offset[oi]);
        Photon ph;
        load_photon(pool, i, ph);
        Rng rng;
        rng_reset(rng);
        for (int q = 0; q < P.n_ops; ++q) apply_op<-1, LAYOUT>(P, q, o, k, rng, ph);
        pool.x[i] = ph.x; pool.y[i] = ph.y; pool.flux[i] = ph.flux;
        pool.dxdz[i] = ph.dxdz; pool.dydz[i] = ph.dydz;
        pool.pupil_u[i] = ph.pu; pool.pupil_v[i] = ph.pv; pool.time[i] = ph.t;
    }
}

// sensor.accumulate(photons, full_image, ...) (photon_pooling.py:195-225)
__global__ __launch_bounds__(256) void k_accumulate(const ims_render_params_t P, const int64_t* __restrict__ photon_offset,
                                                    const ims_photons_t pool, int32_t* __restrict__ pixel_index_out)
{
    const bool silicon = (P.sensor != nullptr) && (P.sensor->kind == IMS_SENSOR_SILICON);
    const bool has_angles = chain_has_angles(P);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pool.n; i += stride) {
        const int32_t oi = pool.obj_index[i];
        const ims_object_t& o = P.objects[oi];
        const int64_t k = o.phot_first + (i - photon_offset[oi]);
        if (pixel_index_out) pixel_index_out[i] = -1;
        Photon ph;
        load_photon(pool, i, ph);
        if (ph.flux == 0.0) continue;
        int ix, iy;
        Rng rng;
        rng_reset(rng);
        if (!land(P, o, k, rng, ph, silicon, has_angles, ix, iy)) continue;
        if (P.realized_flux != nullptr) unsafeAtomicAdd(P.realized_flux + oi, ph.flux);
        bool in_delta = false;
        if (silicon && !(o.flags & IMS_OBJ_FAINT) && (o.bf_state > 0 || P.track_static_delta)) {
            const ims_bf_slot_t bs = P.sensor->bf_slots[slot_index(P, o)];
            const int di = ix - bs.xmin, dj = iy - bs.ymin;
            if (di >= 0 && di < bs.nx && dj >= 0 && dj < bs.ny) {
                unsafeAtomicAdd(P.sensor->bf_delta + (bs.offset + (int64_t)dj * (bs.nx + 1) + di), ph.flux);
                mark_tile_charge(P, bs.offset, bs.nx, di, dj);
                in_delta = P.track_static_delta == 2;
            }
        }
        const int px = ix - P.xmin, py = iy - P.ymin;
        if (px < 0 || px >= P.nx || py < 0 || py >= P.ny) continue;
        const int64_t pidx = (int64_t)py * P.nx + px;
        if (!in_delta) unsafeAtomicAdd(P.image + pidx, ph.flux);
        if (pixel_index_out) pixel_index_out[i] = (int32_t)pidx;
    }
}

// sensor.accumulate for one ROUND of the bright objects: segment-mapped like the fused kernel, but
// the photon (already through the op chain AND the boundary-independent half of the sensor step: the
// `converted` pool format) is loaded from the pool at pool_start[object] + j.
// One workgroup = the photons [j0, j0 + 256) of object `oi` (clipped to j_end).
template <int NV = 0, int WG = 256>
__device__ __forceinline__ void accumulate_segment(const ims_render_params_t& Pg, const ims_photons_t& pool,
                                                   const int64_t* __restrict__ pool_start, int64_t oi, int64_t j0, int64_t j_end,
                                                   const TileLister* lister = nullptr)
{
    const ims_object_t& og = Pg.objects[oi];
    const int64_t left = j_end - j0;                                            // photons of this segment (>= 1)
    const int n_thr = left >= WG ? WG : ((((int)left + 63) >> 6) << 6);
    if ((int)threadIdx.x >= n_thr) return;                                      // photon-less wavefronts leave at once
    const int64_t j = j0 + threadIdx.x;
    // (The prologue of a round's pixel search is a chain of ~17 dependent scalar loads -- the fields of the chain's argument block, of
    // the object row and of the sensor block, each fetched where it is first used, each a cold round trip behind the kernel boundary.
    // Holding them all in one batch with empty asm statements cut the chain to 7 but took the kernel from 94 registers to 128 + 64 ..
    // 156 B of scratch: not kept.  What is kept: the chain of a joint launch found with ONE vector load (joint_chain), and the
    // photon's record requested as soon as its address is known, all four fields at once -- the three others used to wait for the
    // flux -- so that its trip runs beside the rest of the chain: C3 24.08 -> 23.94 ms, C5 6.92 -> 6.83 ms per CCD, round 6.)
    const ims_object_t& o = og;
    const ims_render_params_t& P = Pg;
    const int64_t pstart = pool_start[oi];
    const bool have_sensor = Pg.sensor != nullptr;
    const bool silicon = have_sensor && (P.sensor->kind == IMS_SENSOR_SILICON);
    // the photon's record: all four fields requested before anything of it is looked at (the three others used to wait for the flux)
    const int64_t ip = pstart + (j < j_end ? j : j0);
    const double x0 = pool.x[ip], y0 = pool.y[ip], flux_in = pool.flux[ip], zs = pool.dxdz[ip];
    __shared__ float tile[CT * CT];
    ChargeTile ct;
    PROBE(1);
    tile_begin(tile, ct, P, o, silicon, n_thr, lister);
    PROBE(2);
    PROBE_WG(1, 0);
    double added = 0.0;
    if (j < j_end) {
        int ix, iy;
        // the photon arrives at its conversion depth, diffused (converted pool): only the pixel search is left
        const double flux = flux_in;
        bool ok = false;
        if (flux != 0.0) {
            PROBE(3);
            PROBE_WG(2, 0);
            if (!silicon || (o.flags & IMS_OBJ_FAINT)) {
                ix = (int)floor(x0 + 0.5); iy = (int)floor(y0 + 0.5);
                ok = !(ix < o.stamp_xmin || ix > o.stamp_xmax || iy < o.stamp_ymin || iy > o.stamp_ymax);
            } else {
                const bool coin = __double_as_longlong(zs) < 0;
                ok = land_search<NV, true>(P, o, x0, y0, fabs(zs), coin, ix, iy);
            }
        }
        PROBE(4);
        PROBE_WG(5, 0);
        if (ok) {
            added = flux;
            tile_deposit(tile, ct, P, ix, iy, flux);
        }
    }
    tile_flush(tile, ct, P, n_thr);
    PROBE(6);
    PROBE_WG(7, 0);
    if (P.realized_flux != nullptr) {
        const double tot = wave_sum(added);
        if ((threadIdx.x & 63) == 0 && tot != 0.0) unsafeAtomicAdd(P.realized_flux + oi, tot);
    }
}

// TWO segments of one object per workgroup (photons j0 + t and j0 + 256 + t on thread t): both pool records are requested before
// the first search, so the second photon's record arrives behind the first photon's dependent round trips, and a round has half
// the workgroups to find wave slots for.  The two bodies are written out (a rolled loop lost the register allocation in round 3).
// Same photons, same LDS tile arithmetic (integer counts): the same image bits.  ims_tuning_t.round_two_segments.
template <int NV = 0>
__device__ __forceinline__ void accumulate_segment2(const ims_render_params_t& P, const ims_photons_t& pool,
                                                    const int64_t* __restrict__ pool_start, int64_t oi, int64_t j0, int64_t j_end)
{
    const ims_object_t& o = P.objects[oi];
    const int64_t left = j_end - j0;                                            // photons of this pair of segments (>= 1)
    const int n_thr = left >= 256 ? 256 : ((((int)left + 63) >> 6) << 6);
    if ((int)threadIdx.x >= n_thr) return;                                      // photon-less wavefronts leave at once
    const int64_t ja = j0 + threadIdx.x, jb = ja + 256;
    const bool silicon = (P.sensor != nullptr) && (P.sensor->kind == IMS_SENSOR_SILICON);
    __shared__ float tile[CT * CT];
    ChargeTile ct;
    tile_begin(tile, ct, P, o, silicon, n_thr);
    double added = 0.0;
    const bool has_a = ja < j_end, has_b = jb < j_end;
    const int64_t ia = pool_start[oi] + (has_a ? ja : j0), ib = pool_start[oi] + (has_b ? jb : j0);
    // both records in flight before anything is used
    const double xa = pool.x[ia], ya = pool.y[ia], fa = pool.flux[ia], za = pool.dxdz[ia];
    const double xb = pool.x[ib], yb = pool.y[ib], fb = pool.flux[ib], zb = pool.dxdz[ib];
    const bool plain = !silicon || (o.flags & IMS_OBJ_FAINT);
    if (has_a && fa != 0.0) {
        int ix, iy;
        bool ok;
        if (plain) {
            ix = (int)floor(xa + 0.5); iy = (int)floor(ya + 0.5);
            ok = !(ix < o.stamp_xmin || ix > o.stamp_xmax || iy < o.stamp_ymin || iy > o.stamp_ymax);
        } else ok = land_search<NV, true>(P, o, xa, ya, fabs(za), __double_as_longlong(za) < 0, ix, iy);
        if (ok) { added += fa; tile_deposit(tile, ct, P, ix, iy, fa); }
    }
    if (has_b && fb != 0.0) {
        int ix, iy;
        bool ok;
        if (plain) {
            ix = (int)floor(xb + 0.5); iy = (int)floor(yb + 0.5);
            ok = !(ix < o.stamp_xmin || ix > o.stamp_xmax || iy < o.stamp_ymin || iy > o.stamp_ymax);
        } else ok = land_search<NV, true>(P, o, xb, yb, fabs(zb), __double_as_longlong(zb) < 0, ix, iy);
        if (ok) { added += fb; tile_deposit(tile, ct, P, ix, iy, fb); }
    }
    tile_flush(tile, ct, P, n_thr);
    if (P.realized_flux != nullptr) {
        const double tot = wave_sum(added);
        if ((threadIdx.x & 63) == 0 && tot != 0.0) unsafeAtomicAdd(P.realized_flux + oi, tot);
    }
}

template <int NV>
__global__ __launch_bounds__(256, (NV == 8) ? 2 : 4) void k_accumulate_segments(const ims_render_params_t P, const ims_photons_t pool,
                                                                                const int64_t* __restrict__ pool_start)
{
    const int64_t per = (P.n_segments + N_XCD - 1) / N_XCD;
    const int64_t b = blockIdx.x;
    if ((b / N_XCD) >= per) return;
    const int64_t seg = xcd_segment(b, P.n_segments);
    if (seg >= P.n_segments) return;
    const int64_t oi = P.seg_object ? (int64_t)P.seg_object[seg] : find_object(P.seg_prefix, P.n_objects, seg);
    accumulate_segment<NV>(P, pool, pool_start, oi, (seg - P.seg_prefix[oi]) * P.seg_size, P.objects[oi].n_phot);
}

// The same for objects of at most a wavefront or two of photons (the per-batch shares of photon-pooling mode: median 19):
// ONE WAVEFRONT per object, four independent objects per workgroup, no LDS tile and no barrier -- a share of a few dozen
// photons lands in as many different pixels, so the tile would merge nothing, and a million workgroups of one live
// wavefront each are bound by the dispatch rate (9 ms per batch of C4 for 2 ms of work).  The object index is made
// wave-uniform with readfirstlane so that the row still comes through scalar loads.
template <int NV>
__global__ __launch_bounds__(256, (NV == 8) ? 2 : 5) void k_accumulate_small(const ims_render_params_t P, const ims_photons_t pool,
                                                                             const int64_t* __restrict__ pool_start)
{
    const int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    const int64_t oi = ((int64_t)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)first);
    if (oi >= P.n_objects) return;
    const ims_object_t& o = P.objects[oi];
    const bool silicon = (P.sensor != nullptr) && (P.sensor->kind == IMS_SENSOR_SILICON);
    ChargeTile ct;
    ct.x0 = 0; ct.y0 = 0;
    ct.track = silicon && !(o.flags & IMS_OBJ_FAINT) && (o.bf_state > 0 || P.track_static_delta);
    if (ct.track) ct.slot = P.sensor->bf_slots[slot_index(P, o)];
    const int64_t base = pool_start[oi], n = o.n_phot;
    double added = 0.0;
#pragma unroll 1
    for (int64_t j = threadIdx.x & 63; j < n; j += 64) {
        const int64_t i = base + j;
        const double x0 = pool.x[i], y0 = pool.y[i], flux = pool.flux[i], zs = pool.dxdz[i];
        if (flux == 0.0) continue;
        int ix, iy;
        bool ok;
        if (!silicon || (o.flags & IMS_OBJ_FAINT)) {
            ix = (int)floor(x0 + 0.5); iy = (int)floor(y0 + 0.5);
            ok = !(ix < o.stamp_xmin || ix > o.stamp_xmax || iy < o.stamp_ymin || iy > o.stamp_ymax);
        } else {
            ok = land_search<NV, true>(P, o, x0, y0, fabs(zs), __double_as_longlong(zs) < 0, ix, iy);
        }
        if (ok) {
            added += flux;
            deposit_global(P, ct, ix, iy, flux);
        }
    }
    if (P.realized_flux != nullptr) {
        const double tot = wave_sum(added);
        if ((threadIdx.x & 63) == 0 && tot != 0.0) unsafeAtomicAdd(P.realized_flux + oi, tot);
    }
}

// the round's photons [j0, j_end) of object oi that the object's workgroup `seg` searches (wg photons each); false: none
__device__ __forceinline__ bool round_window(const ims_render_params_t& P, int64_t oi, int64_t seg, int wg, int64_t first, int32_t nrecalc, int64_t& j0, int64_t& j_end)
{
    j0 = first + seg * wg;
    j_end = first + nrecalc;
    const int64_t n = P.objects[oi].n_phot;
    if (j_end > n) j_end = n;
    return j0 < j_end;
}

// The same for round `round` of a chain class whose table holds the objects' FULL photon counts: the round covers the
// photons [round * nrecalc, (round + 1) * nrecalc) of every object, `segs` = ceil(nrecalc / 256) workgroups per object;
// the first n_active rows (sorted by photon count, brightest first) are the objects that reach this round.
// At most 128 VGPRs (4 and 0 vertices; 8 needs the whole file): the rounds share the GPU with the 128-VGPR photon kernels,
// and a wave that needs 136 registers only starts where TWO of those have left a SIMD (measured: the rounds 4 x slower).
template <int NV, int WG = 256>
__global__ __launch_bounds__(WG, (NV == 8) ? 2 : 4) void k_accumulate_round(const ims_render_params_t P, const ims_photons_t pool,
                                                          const int64_t* __restrict__ pool_start, int64_t round_first, int32_t nrecalc,
                                                          int32_t segs)
{
    PROBE(0);
    PROBE_WG(0, 0);
    const int64_t oi = blockIdx.x / segs;
    int64_t j0, j_end;
    if (!round_window(P, oi, (int64_t)(blockIdx.x % segs), WG, round_first, nrecalc, j0, j_end)) return;
    accumulate_segment<NV, WG>(P, pool, pool_start, oi, j0, j_end);
}

// The same with a COMPACT argument block: the pixel search reads a dozen fields of the 1.4-KB launch parameters (object table,
// sensor, image and its bounds, the realized-flux array, the tile tag and slot shift) and four pointers of the pool.  A chain is
// thousands of launches, and HIP's kernel-argument pool holds only so many 1.4-KB blocks: with it full the host enqueues at the
// GPU's pace (25 us of host time per round of a long chain measured) -- which bounds a focal plane of CCDs with long chains.
// The kernel rebuilds the two descriptors in registers (the unused fields vanish), so the body is the one above.
struct RoundArgs {
    const ims_object_t* objects;
    const ims_sensor_t* sensor;
    double* image;
    double* realized_flux;
    const double *px, *py, *pflux, *pz;
    int32_t nx, ny, xmin, ymin;
    uint32_t bf_tag, bf_slot_shift;
    int32_t track_static_delta, pad;
};

// ArgsPtr: the kernel's own argument block, or (joint launches) an entry of a table read through the constant address space
template <class ArgsPtr>
__device__ __forceinline__ void unpack_round_args(ArgsPtr a, ims_render_params_t& P, ims_photons_t& pool)
{
    P.objects = a->objects; P.sensor = a->sensor; P.image = a->image; P.realized_flux = a->realized_flux;
    P.nx = a->nx; P.ny = a->ny; P.xmin = a->xmin; P.ymin = a->ymin;
    P.bf_tag = a->bf_tag; P.bf_slot_shift = a->bf_slot_shift; P.track_static_delta = a->track_static_delta;
    pool.x = const_cast<double*>(a->px); pool.y = const_cast<double*>(a->py); pool.flux = const_cast<double*>(a->pflux);
    pool.dxdz = const_cast<double*>(a->pz);
}

template <int NV, int WG = 256>
__global__ __launch_bounds__(WG, (NV == 8) ? 2 : 4) void k_accumulate_round_c(const RoundArgs a, const int64_t* __restrict__ pool_start,
                                                          int64_t round_first, int32_t nrecalc, int32_t segs)
{
    ims_render_params_t P;
    ims_photons_t pool;
    unpack_round_args(&a, P, pool);
    // (the object index through readfirstlane: the division runs on the vector unit, and the loads of the row are to be scalar loads)
    const int64_t oi = (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)segs));
    int64_t j0, j_end;
    if (!round_window(P, oi, (int64_t)(blockIdx.x % segs), WG, round_first, nrecalc, j0, j_end)) return;
    accumulate_segment<NV, WG>(P, pool, pool_start, oi, j0, j_end);
}

template <int NV>
__global__ __launch_bounds__(256, 4) void k_accumulate_round_c2(const RoundArgs a, const int64_t* __restrict__ pool_start,
                                                                int64_t round_first, int32_t nrecalc, int32_t segs2)
{
    ims_render_params_t P;
    ims_photons_t pool;
    unpack_round_args(&a, P, pool);
    const int64_t oi = blockIdx.x / segs2;
    int64_t j0, j_end;
    if (!round_window(P, oi, (int64_t)(blockIdx.x % segs2), 512, round_first, nrecalc, j0, j_end)) return;
    accumulate_segment2<NV>(P, pool, pool_start, oi, j0, j_end);
}

// ---- JOINT rounds: the same round of the top chains of several CCDs in one launch ----
// A focal plane's CCDs are independent renders (own sensor state, image, pool, object table), and with a bright tail each is
// bound by the dependent rounds of its brightest star -- hundreds of launches of a few dozen workgroups.  Chains of different
// CCDs on different streams barely overlap on this device (four side by side 108 - 150 ms against 158 ms
// one after the other), while one launch that holds the round of MANY objects costs little more than the round of one (C3: 41
// objects 2.8 x one star).  So the launch takes the argument blocks of up to IMS_JOINT_MAX chains by value and a workgroup
// finds its chain from the ascending workgroup ends (scalar compares on kernel arguments); the body is the one above.
struct JointEnds { int32_t v[IMS_JOINT_MAX]; };      // ascending workgroup ends of the chains of one launch (a chain that sits out: zero width)

struct JointAcc {                           // per chain, constant over the rounds: lives in device memory (ims_plans_run_joint)
    RoundArgs a[IMS_JOINT_MAX];
    const int64_t* pool_start[IMS_JOINT_MAX];
    const int64_t* tile_prefix[IMS_JOINT_MAX];      // search-side lists (TileLister): tiles before each slot of the class,
    unsigned int* words[IMS_JOINT_MAX];             // the chain's tile words,
    int32_t first_slot[IMS_JOINT_MAX];              // and the class's first slot
};
typedef const JointAcc __attribute__((address_space(4))) * ConstAcc;        // (uniform addresses: scalar loads whatever the kernel stores)

// The tables of ONE round of a joint run -- workgroup ends of the pixel search (ea), tile ends (eu), regions that go on (ns),
// workgroup ends of the list builder (ewg), tiles per chain (tof) -- live in DEVICE memory, all rounds of the run uploaded at
// once (ims_plans_run_joint), and a launch takes a pointer to its round's block.  (By value they were 128 .. 768 bytes of
// kernel arguments per launch, four launches per round, thousands of rounds per batch, and would have doubled with 64 chains
// per run.)  Read through the constant address space: uniform addresses, scalar loads.
struct JointRound { JointEnds ea, eu, ns, ewg, tof; };
typedef const JointEnds __attribute__((address_space(4))) * ConstEnds;

// which chain workgroup b belongs to: the number of ends <= b.  One entry per lane (a single 256-byte load), a ballot and a population
// count: ONE round trip at the head of every round kernel, where 63 scalar compares on four batches of scalar loads were three
// (the registers do not hold 64 ends at once) -- behind a kernel boundary every trip of the prologue is a cold one (round 6).
// All 64 lanes must be active.
__device__ __forceinline__ int joint_chain(const JointEnds* e_global, int& b)
{
    const int lane = (int)(threadIdx.x & 63);
    const int v = e_global->v[lane];
    const int c = (int)__popcll(__builtin_amdgcn_ballot_w64(lane < IMS_JOINT_MAX - 1 && b >= v));
    if (c > 0) b -= __builtin_amdgcn_readlane(v, c - 1);
    return c;
}
__device__ __forceinline__ int joint_entry(const JointEnds* e_global, int c) { return ((ConstEnds)(uintptr_t)e_global)->v[c]; }

__device__ __forceinline__ TileListerChain lister_chain(const TileLister& L, int slot_idx)
{
    ConstAcc Jc = (ConstAcc)(uintptr_t)L.J;
    TileListerChain C;
    C.lo = slot_idx - Jc->first_slot[L.chain];
    C.tile_base = Jc->tile_prefix[L.chain][C.lo];
    C.words = Jc->words[L.chain];
    C.on = C.tile_base < joint_entry(&L.R->tof, L.chain);          // (regions are in the order of their chains' lengths)
    return C;
}

template <int NV, int WG = 256>
__global__ __launch_bounds__(WG, (NV == 8) ? 2 : 4) void k_accumulate_round_j(const JointAcc* __restrict__ J, const JointRound* __restrict__ R,
                                                                              uint32_t tag, int64_t round_first, int32_t nrecalc, int32_t segs,
                                                                              unsigned long long* list, int* list_count, unsigned int round_word)
{
    int b = (int)blockIdx.x;
    const int c = joint_chain(&R->ea, b);
    // the table through the CONSTANT address space: its loads at uniform addresses are scalar loads whatever the kernel stores
    // (through a plain pointer the twelve fields sit in vector registers for the whole body: 128 + spills instead of 92)
    ConstAcc Jc = (ConstAcc)(uintptr_t)J;
    ims_render_params_t P;
    ims_photons_t pool;
    unpack_round_args(&Jc->a[c], P, pool);
    P.bf_tag = tag; P.bf_slot_shift = 0;
    const int64_t* pool_start = Jc->pool_start[c];
    const int64_t oi = b / segs;
    int64_t j0, j_end;
    if (!round_window(P, oi, (int64_t)(b % segs), WG, round_first, nrecalc, j0, j_end)) return;
    TileLister tl;
    tl.list = list; tl.count = list_count; tl.round_word = round_word; tl.chain = c; tl.J = J; tl.R = R;
    accumulate_segment<NV, WG>(P, pool, pool_start, oi, j0, j_end, &tl);
}

// Which slot of a range does block b work on: the last k with prefix[k] <= b (prefix = ascending tile offsets of the slots,
// prefix[0] = 0).  A bisection is log2(n) DEPENDENT loads at the head of every tile kernel -- 6 for the 41 regions of the
// long chains, 11 for the 1 550 of the middle class, each a cold-L2 round trip of ~1.4 us in a kernel that runs for 6 - 30 us.
// Here the wavefront looks at 64 entries at a time (one load per lane, a ballot, a population count): one load for up to 64
// slots, two up to 4 096.  Every wavefront of the workgroup computes the same (uniform) answer; all 64 lanes must be active.
__device__ __forceinline__ int find_slot(const int64_t* __restrict__ prefix, int n_slots, int64_t b)
{
    const int lane = threadIdx.x & 63;
    int base = 0, n = n_slots;
    while (n > 64) {
        const int stride = (n + 63) >> 6;
        const int k = lane * stride;
        const bool le = k < n && prefix[base + k] <= b;
        const int cnt = __popcll(__builtin_amdgcn_ballot_w64(le));       // entries 0, stride, 2 stride, ... <= b form a prefix
        const int first = (cnt - 1) * stride;
        base += first;
        n = (n - first < stride) ? n - first : stride;
    }
    const bool le = lane < n && prefix[base + lane] <= b;
    return base + __popcll(__builtin_amdgcn_ballot_w64(le)) - 1;
}

// ---------------- Silicon boundary state ----------------
__device__ __forceinline__ void empty_owned(const ims_sensor_t& s, int n, double& x, double& y)
{
    const int nV = s.num_vertices;
    if (n == 0) { x = 0.0; y = 0.0; return; }
    if (n <= nV) { x = s.emptypoly[2 * n]; y = 0.0; return; }
    if (n == nV + 1) { x = 1.0; y = 0.0; return; }
    const int m = n - nV - 2;
    x = 0.0; y = s.emptypoly[2 * (1 + m)];
}

// What the tree-ring closed form needs of the sensor block, read ONCE per thread.  (Read through `s` at every evaluation, the
// stores in between -- the state arrays hang off the same block -- made the compiler reload the block and redo everything that
// depends on tr_dr alone: the Newton steps of 1 / tr_dr and the IEEE division tr_dr^2 / 6, ~30 of an evaluation's ~115 VALU
// instructions, twenty evaluations per cell in k_init_tiles; SQ_INSTS_VALU of round 5: the initial state was 24 % of a focal
// plane's VALU work.)  Same operations on the same operands: same bits.
struct TreeRing {
    double dr, dr_y, h2, cx, cy;
    const double* table;
    const double* table2;
    int n;
};

__device__ __forceinline__ TreeRing treering_of(const ims_sensor_t& s)
{
    TreeRing T;
    T.n = s.n_tr; T.dr = s.tr_dr; T.cx = s.tr_cx; T.cy = s.tr_cy; T.table = s.tr_table; T.table2 = s.tr_table2;
    T.dr_y = 0.0; T.h2 = 0.0;
    if (T.n > 0) {
        // the part of ddiv(r, dr) that does not depend on r (ims_math.h: two Newton steps on the reciprocal seed)
        double y = __builtin_amdgcn_rcp(T.dr);
        double e = fma(-T.dr, y, 1.0);
        y = fma(y, e, y);
        e = fma(-T.dr, y, 1.0);
        T.dr_y = fma(y, e, y);
        T.h2 = T.dr * T.dr / 6.0;
    }
    return T;
}

__device__ __forceinline__ double treering_shift(const TreeRing& T, double r)
{
    if (T.n <= 0) return 0.0;
    // ddiv(r, dr) with the reciprocal prepared above
    const double q = r * T.dr_y;
    const double rem = fma(-T.dr, q, r);
    const double f = fma(rem, T.dr_y, q);
    if (!(f > 0.0) || f >= (double)(T.n - 1)) return 0.0;
    const int i = (int)f;
    const double b = f - (double)i;
    const double v0 = T.table[i], v1 = T.table[i + 1];
    if (T.table2 == nullptr) return v0 + b * (v1 - v0);
    const double a = 1.0 - b;
    return a * v0 + b * v1 + ((a * a * a - a) * T.table2[i] + (b * b * b - b) * T.table2[i + 1]) * T.h2;
}

// The boundary kernels run over a RANGE of slots in one launch: thread -> global owner cell ->
// slot by binary search over the packed cell offsets (wave-uniform except at slot seams).
struct CellRef { SlotView sl; int i, j; int64_t c; bool valid; };

__device__ __forceinline__ CellRef locate_cell(const ims_sensor_t& s, int first_slot, int n_slots, int64_t cell_begin,
                                               int64_t cell_count)
{
    CellRef r;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    r.valid = t < cell_count;
    if (!r.valid) return r;
    const int64_t g = cell_begin + t;
    int lo = first_slot, hi = first_slot + n_slots;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.bf_slots[mid].offset <= g) lo = mid; else hi = mid;
    }
    const ims_bf_slot_t bs = s.bf_slots[lo];
    r.sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    r.c = g - bs.offset;
    r.i = (int)(r.c % (bs.nx + 1));
    r.j = (int)(r.c / (bs.nx + 1));
    return r;
}

// owned boundary point n of owner cell (ci, cj) in its undistorted-plus-tree-ring state (pixel-local coordinates)
__device__ __forceinline__ void init_point(const ims_sensor_t& s, const TreeRing& T, const SlotView& sl, int ci, int cj, int n,
                                           double& px, double& py)
{
    double ex, ey;
    empty_owned(s, n, ex, ey);
    const double tx = ((double)(sl.xmin + ci) - 0.5 + ex) - T.cx;
    const double ty = ((double)(sl.ymin + cj) - 0.5 + ey) - T.cy;
    const double rr = dsqrt0(tx * tx + ty * ty);
    const double sh = treering_shift(T, rr);
    px = ex; py = ey;
    if (rr > 0.0 && sh != 0.0) { px = ex + ddiv(sh * tx, rr); py = ey + ddiv(sh * ty, rr); }
}

// Initial state of a range of slots: boundary points, zero delta charge AND the bounds line of every pixel.
// The bounds need the points of the right and upper neighbour cells; they are recomputed here from the same
// closed form (bit-identical to what those cells store) instead of being read back in a second pass.
__global__ __launch_bounds__(256) void k_init_boundaries(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                         int64_t cell_begin, int64_t cell_count)
{
    const ims_sensor_t& s = *sp;
    const CellRef r = locate_cell(s, first_slot, n_slots, cell_begin, cell_count);
    if (!r.valid) return;
    const SlotView& sl = r.sl;
    const TreeRing T = treering_of(s);
    const int nV = s.num_vertices, npo = 2 * nV + 2, nv = 4 * nV + 4;
    double* pts = s.bf_boundary + (sl.offset + r.c) * npo * 2;
    for (int n = 0; n < npo; ++n) {
        double px, py;
        init_point(s, T, sl, r.i, r.j, n, px, py);
        pts[2 * n] = px; pts[2 * n + 1] = py;
    }
    s.bf_delta[sl.offset + r.c] = 0.0;
    const int i = r.i, j = r.j;
    if (i >= sl.nx || j >= sl.ny) return;
    double ixmin = 0.0, ixmax = 1.0, iymin = 0.0, iymax = 1.0;
    double oxmin = 0.0, oxmax = 1.0, oymin = 0.0, oymax = 1.0;
    double v0x = 0.0;
    for (int k = 0; k < nv; ++k) {
        // same vertex -> (cell, owned point) map as polygon_vertex
        int ci = i, cj = j, q;
        double ax = 0.0, ay = 0.0;
        if (k <= nV + 1) { q = k; }
        else if (k <= 2 * nV + 1) { ci = i + 1; ax = 1.0; q = nV + 2 + (k - nV - 2); }
        else if (k <= 3 * nV + 3) { cj = j + 1; ay = 1.0; q = nV + 1 - (k - 2 * nV - 2); }
        else { q = nV + 2 + (nV - 1 - (k - 3 * nV - 4)); }
        double vx, vy;
        init_point(s, T, sl, ci, cj, q, vx, vy);
        vx = vx + ax; vy = vy + ay;
        if (k == 0) v0x = vx;
        if (vx < oxmin) oxmin = vx;
        if (vx > oxmax) oxmax = vx;
        if (vy < oymin) oymin = vy;
        if (vy > oymax) oymax = vy;
        if (k <= nV + 1) { if (vy > iymin) iymin = vy; }
        if (k >= nV + 1 && k <= 2 * nV + 2) { if (vx < ixmax) ixmax = vx; }
        if (k >= 2 * nV + 2 && k <= 3 * nV + 3) { if (vy < iymax) iymax = vy; }
        if (k >= 3 * nV + 3) { if (vx > ixmin) ixmin = vx; }
    }
    if (v0x > ixmin) ixmin = v0x;
    double* b = s.bf_bounds + (sl.offset + r.c) * 8;
    b[0] = ixmin; b[1] = ixmax; b[2] = iymin; b[3] = iymax;
    b[4] = oxmin; b[5] = oxmax; b[6] = oymin; b[7] = oymax;
}

// The same initial state, one 16 x 16 tile of owner cells per workgroup (grid.y = slot of the range, grid.x = tile; 4
// vertices per edge): every lane evaluates the ten owned points of ITS cell once, hands the left-edge and bottom-row
// points its left / lower neighbours need through LDS, and only the lanes at the right / upper rim of the tile evaluate
// their neighbour's points themselves -- ~12 evaluations of the tree-ring closed form per cell instead of 30 (each is a
// sqrt, two divisions and a spline).  Same function of (cell, point), so the same bits as k_init_boundaries.
constexpr int UT = 16;            // tile edge of the boundary kernels (mark_tile_charge assumes 16)
__host__ __device__ __forceinline__ int tiles_across(int n) { return (n + 1 + UT - 1) / UT; }   // tiles across the n + 1 owner cells of a slot's row / column
constexpr int IT_NV = 4, IT_NPO = 2 * IT_NV + 2, IT_NVT = 4 * IT_NV + 4;

// tile_prefix (device, prefix sum of the tiles of the slots first_slot ..): a 1-D grid over exactly the tiles of the
// range, block -> (slot, tile) by binary search as in the update kernels; NULL: grid.y = slot, grid.x = tile of the slot
// (blocks beyond the slot's tiles leave).
__global__ __launch_bounds__(256) void k_init_tiles(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                    const int64_t* __restrict__ tile_prefix)
{
    // the owned points of the tile's cells in the order of the global array -- [row][cell][point], ten double2 per cell --
    // so that they go out as contiguous runs (a lane that stored its own ten points wrote 16 bytes every 160: 64 requests
    // per store instruction; 2.16 ms for the 16.8 M cells of a CCD, 1.8 TB/s of the bytes written).  The bounds lines reuse
    // the buffer for the same reason.
    __shared__ double2 P[UT * UT * IT_NPO];
    const ims_sensor_t& s = *sp;
    int slot = first_slot + (int)blockIdx.y, t = (int)blockIdx.x;
    if (tile_prefix != nullptr) {
        const int64_t b = blockIdx.x;
        const int lo = find_slot(tile_prefix, n_slots, b);
        slot = first_slot + lo;
        t = (int)(b - tile_prefix[lo]);
    }
    const ims_bf_slot_t bs = s.bf_slots[slot];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx), tiles_y = tiles_across(sl.ny);
    if (t >= tiles_x * tiles_y) return;
    const TreeRing T = treering_of(s);
    const int lx = threadIdx.x % UT, ly = threadIdx.x / UT;
    const int tx0 = (t % tiles_x) * UT, ty0 = (t / tiles_x) * UT;
    const int i = tx0 + lx, j = ty0 + ly;
    const bool owner = (i <= sl.nx && j <= sl.ny);
    double2 own[IT_NPO];
    if (owner) {
#pragma unroll
        for (int n = 0; n < IT_NPO; ++n) {
            init_point(s, T, sl, i, j, n, own[n].x, own[n].y);
            P[(ly * UT + lx) * IT_NPO + n] = own[n];
        }
        s.bf_delta[cell_index(sl, i, j)] = 0.0;
    }
    __syncthreads();
    // points out: row ly of the tile is one contiguous run of (cells of the slot in that row) x ten double2
    {
        const int ncx = (sl.nx + 1 - tx0 < UT) ? sl.nx + 1 - tx0 : UT;           // owner cells per row of this tile
        const int nrow = (sl.ny + 1 - ty0 < UT) ? sl.ny + 1 - ty0 : UT;
#pragma unroll
        for (int e = (int)threadIdx.x; e < UT * UT * IT_NPO; e += 256) {
            const int r = e / (UT * IT_NPO), k = e - r * (UT * IT_NPO);
            if (r < nrow && k < ncx * IT_NPO)
                ((double2*)(s.bf_boundary + cell_index(sl, tx0, ty0 + r) * IT_NPO * 2))[k] = P[e];
        }
    }
    const bool inner = owner && i < sl.nx && j < sl.ny;                           // a pixel: has a bounds line
    // The points of the cells just outside the tile, which the pixels at its right / upper rim need, evaluated by the wavefront
    // TOGETHER (a wavefront is four rows of sixteen cells): the four left-edge points of the cell right of a row by the row's
    // lanes 12 .. 15, one each, handed to lane 15 by shuffles; the six bottom-row points of the cells above the tile by the
    // four rows of its last wavefront, two rounds.  (Each rim lane evaluating its own -- four and six evaluations that the whole
    // wavefront sits through -- made 14 / 20 evaluations per wavefront where 11 / 13 do: the closed form is most of this kernel.)
    static_assert(IT_NV == 4 && UT == 16, "the rim exchange below is written for 4 vertices per edge and 16 x 16 tiles");
    double2 rgt_rim[IT_NV], upp_rim[IT_NV + 2];
    {
        const int lane = (int)(threadIdx.x & 63), row_base = lane & ~15;
        double2 rr;
        init_point(s, T, sl, tx0 + UT, j, IT_NV + 2 + (lx & 3), rr.x, rr.y);
#pragma unroll
        for (int m = 0; m < IT_NV; ++m) { rgt_rim[m].x = __shfl(rr.x, row_base + 12 + m, 64); rgt_rim[m].y = __shfl(rr.y, row_base + 12 + m, 64); }
#pragma unroll
        for (int q = 0; q <= IT_NV + 1; ++q) upp_rim[q] = make_double2(0.0, 0.0);
        if (threadIdx.x >= 192) {                                                    // rows 12 .. 15: wave-uniform
            const int r = ly - 12;
            double2 ua, ub;
            init_point(s, T, sl, i, ty0 + UT, r, ua.x, ua.y);
            init_point(s, T, sl, i, ty0 + UT, 4 + (r & 1), ub.x, ub.y);
#pragma unroll
            for (int q = 0; q < 4; ++q) { upp_rim[q].x = __shfl(ua.x, lx + 16 * q, 64); upp_rim[q].y = __shfl(ua.y, lx + 16 * q, 64); }
#pragma unroll
            for (int q = 0; q < 2; ++q) { upp_rim[4 + q].x = __shfl(ub.x, lx + 16 * q, 64); upp_rim[4 + q].y = __shfl(ub.y, lx + 16 * q, 64); }
        }
    }
    double bnd[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (inner) {
        // the right neighbour's left edge and the upper neighbour's bottom row: from LDS inside the tile, from the exchange at its rim
        double2 rgt[IT_NV], upp[IT_NV + 2];
        if (lx + 1 < UT) {
#pragma unroll
            for (int m = 0; m < IT_NV; ++m) rgt[m] = P[(ly * UT + lx + 1) * IT_NPO + IT_NV + 2 + m];
        } else {
#pragma unroll
            for (int m = 0; m < IT_NV; ++m) rgt[m] = rgt_rim[m];
        }
        if (ly + 1 < UT) {
#pragma unroll
            for (int q = 0; q <= IT_NV + 1; ++q) upp[q] = P[((ly + 1) * UT + lx) * IT_NPO + q];
        } else {
#pragma unroll
            for (int q = 0; q <= IT_NV + 1; ++q) upp[q] = upp_rim[q];
        }
        double ixmin = 0.0, ixmax = 1.0, iymin = 0.0, iymax = 1.0;
        double oxmin = 0.0, oxmax = 1.0, oymin = 0.0, oymax = 1.0;
        double v0x = 0.0;
#pragma unroll
        for (int k = 0; k < IT_NVT; ++k) {
            // same vertex -> (cell, owned point) map as polygon_vertex
            double vx, vy;
            if (k <= IT_NV + 1) { vx = own[k].x; vy = own[k].y; }
            else if (k <= 2 * IT_NV + 1) { vx = rgt[k - IT_NV - 2].x + 1.0; vy = rgt[k - IT_NV - 2].y; }
            else if (k <= 3 * IT_NV + 3) { vx = upp[IT_NV + 1 - (k - 2 * IT_NV - 2)].x; vy = upp[IT_NV + 1 - (k - 2 * IT_NV - 2)].y + 1.0; }
            else { vx = own[IT_NV + 2 + (IT_NV - 1 - (k - 3 * IT_NV - 4))].x; vy = own[IT_NV + 2 + (IT_NV - 1 - (k - 3 * IT_NV - 4))].y; }
            if (k == 0) v0x = vx;
            if (vx < oxmin) oxmin = vx;
            if (vx > oxmax) oxmax = vx;
            if (vy < oymin) oymin = vy;
            if (vy > oymax) oymax = vy;
            if (k <= IT_NV + 1) { if (vy > iymin) iymin = vy; }
            if (k >= IT_NV + 1 && k <= 2 * IT_NV + 2) { if (vx < ixmax) ixmax = vx; }
            if (k >= 2 * IT_NV + 2 && k <= 3 * IT_NV + 3) { if (vy < iymax) iymax = vy; }
            if (k >= 3 * IT_NV + 3) { if (vx > ixmin) ixmin = vx; }
        }
        if (v0x > ixmin) ixmin = v0x;
        bnd[0] = ixmin; bnd[1] = ixmax; bnd[2] = iymin; bnd[3] = iymax;
        bnd[4] = oxmin; bnd[5] = oxmax; bnd[6] = oymin; bnd[7] = oymax;
    }
    __syncthreads();                                   // everybody has read its neighbours' points: the buffer is free
    if (inner) {
#pragma unroll
        for (int q = 0; q < 4; ++q) P[(ly * UT + lx) * 4 + q] = make_double2(bnd[2 * q], bnd[2 * q + 1]);
    }
    __syncthreads();
    {
        const int ncx = (sl.nx - tx0 < UT) ? sl.nx - tx0 : UT;                   // pixels per row of this tile (may be <= 0)
        const int nrow = (sl.ny - ty0 < UT) ? sl.ny - ty0 : UT;
#pragma unroll
        for (int e = (int)threadIdx.x; e < UT * UT * 4; e += 256) {
            const int r = e / (UT * 4), k = e - r * (UT * 4);
            if (r < nrow && k < ncx * 4)
                ((double2*)(s.bf_bounds + cell_index(sl, tx0, ty0 + r) * 8))[k] = P[e];
        }
    }
}

// ---- slot 0 without stored state (ims_render_params_t.lazy_static): the photons the fused launch set aside ----
// Pixel (i, j) of slot 0 in its initial state, evaluated where it is needed: the ten owned points of its cell, the four left-edge
// points of the cell to the right, the six bottom-row points of the cell above -- init_point, the function k_init_tiles stores --
// and from them the bounds line as k_init_tiles forms it.  4 vertices per edge.
struct LazyPixel { double2 own[IT_NPO], rgt[IT_NV], upp[IT_NV + 2]; double b[8]; };

__device__ __forceinline__ void lazy_pixel(const ims_sensor_t& s, const TreeRing& T, const SlotView& sl, int i, int j, LazyPixel& px)
{
#pragma unroll
    for (int n = 0; n < IT_NPO; ++n) init_point(s, T, sl, i, j, n, px.own[n].x, px.own[n].y);
#pragma unroll
    for (int m = 0; m < IT_NV; ++m) init_point(s, T, sl, i + 1, j, IT_NV + 2 + m, px.rgt[m].x, px.rgt[m].y);
#pragma unroll
    for (int q = 0; q <= IT_NV + 1; ++q) init_point(s, T, sl, i, j + 1, q, px.upp[q].x, px.upp[q].y);
    double ixmin = 0.0, ixmax = 1.0, iymin = 0.0, iymax = 1.0;
    double oxmin = 0.0, oxmax = 1.0, oymin = 0.0, oymax = 1.0;
    double v0x = 0.0;
#pragma unroll
    for (int k = 0; k < IT_NVT; ++k) {
        double vx, vy;
        if (k <= IT_NV + 1) { vx = px.own[k].x; vy = px.own[k].y; }
        else if (k <= 2 * IT_NV + 1) { vx = px.rgt[k - IT_NV - 2].x + 1.0; vy = px.rgt[k - IT_NV - 2].y; }
        else if (k <= 3 * IT_NV + 3) { vx = px.upp[IT_NV + 1 - (k - 2 * IT_NV - 2)].x; vy = px.upp[IT_NV + 1 - (k - 2 * IT_NV - 2)].y + 1.0; }
        else { vx = px.own[IT_NV + 2 + (IT_NV - 1 - (k - 3 * IT_NV - 4))].x; vy = px.own[IT_NV + 2 + (IT_NV - 1 - (k - 3 * IT_NV - 4))].y; }
        if (k == 0) v0x = vx;
        if (vx < oxmin) oxmin = vx;
        if (vx > oxmax) oxmax = vx;
        if (vy < oymin) oymin = vy;
        if (vy > oymax) oymax = vy;
        if (k <= IT_NV + 1) { if (vy > iymin) iymin = vy; }
        if (k >= IT_NV + 1 && k <= 2 * IT_NV + 2) { if (vx < ixmax) ixmax = vx; }
        if (k >= 2 * IT_NV + 2 && k <= 3 * IT_NV + 3) { if (vy < iymax) iymax = vy; }
        if (k >= 3 * IT_NV + 3) { if (vx > ixmin) ixmin = vx; }
    }
    if (v0x > ixmin) ixmin = v0x;
    px.b[0] = ixmin; px.b[1] = ixmax; px.b[2] = iymin; px.b[3] = iymax;
    px.b[4] = oxmin; px.b[5] = oxmax; px.b[6] = oymin; px.b[7] = oymax;
}

// polygon_test (ims_photon.h) on the evaluated points: the same vertices in the same order through the same arithmetic
__device__ __forceinline__ bool lazy_polygon_test(const ims_sensor_t& s, const LazyPixel& px, double x, double y, double zfactor)
{
    const bool scaled = (zfactor != 1.0);
    bool inside = false;
    double lx, ly;
    {
        constexpr int k = IT_NVT - 1;                                                    // closing vertex: own left edge, first point
        lx = px.own[5 * IT_NV + 5 - k].x; ly = px.own[5 * IT_NV + 5 - k].y;
        if (scaled) {
            const double ex = s.emptypoly[2 * k], ey = s.emptypoly[2 * k + 1];
            lx = ex + (lx - ex) * zfactor;
            ly = ey + (ly - ey) * zfactor;
        }
    }
#pragma unroll
    for (int k = 0; k < IT_NVT; ++k) {
        double kx, ky;
        if (k <= IT_NV + 1) { kx = px.own[k].x; ky = px.own[k].y; }
        else if (k <= 2 * IT_NV + 1) { kx = px.rgt[k - IT_NV - 2].x + 1.0; ky = px.rgt[k - IT_NV - 2].y + 0.0; }
        else if (k <= 3 * IT_NV + 3) { kx = px.upp[3 * IT_NV + 3 - k].x + 0.0; ky = px.upp[3 * IT_NV + 3 - k].y + 1.0; }
        else { kx = px.own[5 * IT_NV + 5 - k].x; ky = px.own[5 * IT_NV + 5 - k].y; }
        if (scaled) {
            const double ex = s.emptypoly[2 * k], ey = s.emptypoly[2 * k + 1];
            kx = ex + (kx - ex) * zfactor;
            ky = ey + (ky - ey) * zfactor;
        }
        if ((ky > y) != (ly > y)) {
            const double dy = ly - ky;
            const double lhs = (x - kx) * dy, rhs = (lx - kx) * (y - ky);
            if ((dy > 0.0) ? (lhs < rhs) : (lhs > rhs)) inside = !inside;
        }
        lx = kx; ly = ky;
    }
    return inside;
}

// inside_pixel (ims_photon.h) for slot 0 without stored state; z: the conversion depth
__device__ __forceinline__ bool lazy_inside_pixel(const ims_sensor_t& s, const TreeRing& T, const SlotView& sl, int ix, int iy, double x, double y,
                                                  double z, bool want_edge, bool& off_edge)
{
    const int i = ix - sl.xmin, j = iy - sl.ymin;
    if (i < 0 || i >= sl.nx || j < 0 || j >= sl.ny) {
        if (want_edge) off_edge = true;
        return false;
    }
    LazyPixel px;
    lazy_pixel(s, T, sl, i, j, px);
    bool inside;
    if (x > px.b[0] && x < px.b[1] && y > px.b[2] && y < px.b[3]) inside = true;
    else if (!(x >= px.b[4] && x <= px.b[5] && y >= px.b[6] && y <= px.b[7])) inside = false;
    else inside = lazy_polygon_test(s, px, x, y, dtanh_pos(ddiv(z, 12.0)));
    if (!inside && want_edge) {
        off_edge = false;
        if (i == 0 && x < px.b[0]) off_edge = true;
        if (i == sl.nx - 1 && x > px.b[1]) off_edge = true;
        if (j == 0 && y < px.b[2]) off_edge = true;
        if (j == sl.ny - 1 && y > px.b[3]) off_edge = true;
    }
    return inside;
}

// The photons ims_shoot_accumulate set aside (margin_append): land_search from the point where it would have read the state.
// A neighbour whose outer bounds cannot hold the point is not evaluated: no vertex of a pristine polygon lies further than
// pristine_margin from its nominal place, so outer bounds lie within [-m, 1 + m] -- the candidates of the walk are the same.
__device__ __forceinline__ void margin_photon(const ims_render_params_t& P, const ims_sensor_t& s, const TreeRing& T, const SlotView& sl, double mm,
                                              int64_t r)
{
    const double* rec = P.margin_list + 5 * (size_t)r;
    const double x0 = rec[0], y0 = rec[1], zs = rec[2], flux = rec[3];
    const int64_t oi = __double_as_longlong(rec[4]);
    const ims_object_t& o = P.objects[oi];
    const double z = fabs(zs);
    const bool coin = __double_as_longlong(zs) < 0;
    int ix = (int)floor(x0 + 0.5), iy = (int)floor(y0 + 0.5);
    const double x = x0 - (double)ix + 0.5, y = y0 - (double)iy + 0.5;
    bool off_edge = false;
    bool found = lazy_inside_pixel(s, T, sl, ix, iy, x, y, z, true, off_edge);
    if (!found && off_edge) return;
    int step = 0;
    if (!found) {
        step = search_step(x, y);
        for (int m = 1; m < 9; ++m) {
            const int nb = ((m * step - 1) & 7) + 1;
            const int jx = ix + xoff(nb), jy = iy + yoff(nb);
            const int i = jx - sl.xmin, j = jy - sl.ymin;
            if (i < 0 || i >= sl.nx || j < 0 || j >= sl.ny) continue;
            const double xb = x - (double)xoff(nb), yb = y - (double)yoff(nb);
            if (xb < -mm || xb > 1.0 + mm || yb < -mm || yb > 1.0 + mm) continue;
            LazyPixel px;
            lazy_pixel(s, T, sl, i, j, px);
            if (!(xb >= px.b[4] && xb <= px.b[5] && yb >= px.b[6] && yb <= px.b[7])) continue;      // not a candidate of the walk
            bool in = (xb > px.b[0] && xb < px.b[1] && yb > px.b[2] && yb < px.b[3]);
            if (!in) in = lazy_polygon_test(s, px, xb, yb, dtanh_pos(ddiv(z, 12.0)));
            if (in) { ix = jx; iy = jy; found = true; break; }
        }
    }
    if (!found) {
        const int nb = coin ? 0 : step;
        ix = ix + xoff(nb); iy = iy + yoff(nb);
    }
    if (ix < o.stamp_xmin || ix > o.stamp_xmax || iy < o.stamp_ymin || iy > o.stamp_ymax) return;
    const int pxl = ix - P.xmin, pyl = iy - P.ymin;
    if (pxl >= 0 && pxl < P.nx && pyl >= 0 && pyl < P.ny) unsafeAtomicAdd(P.image + ((int64_t)pyl * P.nx + pxl), flux);
    if (P.realized_flux != nullptr) unsafeAtomicAdd(P.realized_flux + oi, flux);
}

// A workgroup takes 2 048 places of the list at a time (the wavefronts' octets, then the overflow region), collects the filled ones
// in LDS -- one place in six is -- and then works on them with every lane busy (a lane per place sat through the search with a sixth
// of its lanes: 0.97 ms for C3's launch where 0.25 do).  The order of the photons does not matter: integer counts, atomics.
constexpr int MARGIN_CHUNK = 2048;
__global__ __launch_bounds__(256, 2) void k_margin_photons(const ims_render_params_t P)
{
    __shared__ int q[MARGIN_CHUNK];
    __shared__ int qn;
    const ims_sensor_t& s = *P.sensor;
    const TreeRing T = treering_of(s);
    const ims_bf_slot_t bs = s.bf_slots[0];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const double mm = s.pristine_margin;
    unsigned int n_over = (unsigned int)P.margin_count[0];
    if (n_over > P.margin_cap) n_over = P.margin_cap;
    const int64_t n_oct = P.margin_waves * 8, n = n_oct + (int64_t)n_over;
    for (int64_t c0 = (int64_t)blockIdx.x * MARGIN_CHUNK; c0 < n; c0 += (int64_t)gridDim.x * MARGIN_CHUNK) {
        if (threadIdx.x == 0) qn = 0;
        __syncthreads();
        for (int k = (int)threadIdx.x; k < MARGIN_CHUNK; k += 256) {
            const int64_t r = c0 + k;
            const bool filled = r < n && (r >= n_oct || (int)(r & 7) < (int)P.margin_wave_count[r >> 3]);
            if (filled) q[atomicAdd(&qn, 1)] = k;
        }
        __syncthreads();
        const int m = qn;
        for (int k = (int)threadIdx.x; k < m; k += 256) margin_photon(P, s, T, sl, mm, c0 + q[k]);
        __syncthreads();
    }
}

__device__ __forceinline__ int owned_to_vertex(int nV, int n)
{
    if (n <= nV + 1) return n;
    const int m = n - nV - 2;
    return 3 * nV + 4 + (nV - 1 - m);
}

// Silicon::updatePixelDistortions.  One 16x16 workgroup per tile of owner cells of one slot: the
// delta-charge halo tile ((16+2q+1)^2 doubles) is staged in LDS once, then every thread gathers its
// charged neighbours from LDS in a FIXED order (so the result is bit-reproducible) and adds the
// scaled tabulated displacements to the boundary points it owns.  A per-cell `changed` byte lets
// k_refresh_changed skip pixels whose polygon did not move.
constexpr int UQMAX = 4;          // largest supported qdist
constexpr int UH = UT + 2 * UQMAX + 1;

// no charge was deposited (with this tag) within reach of tile (tx, ty): nothing can move there
__device__ __forceinline__ bool tile_out_of_reach(const ims_sensor_t& s, const SlotView& sl, int tx, int ty, unsigned int tag)
{
    if (tag == 0u || s.bf_tile_charge == nullptr) return false;
    const int tiles_x = tiles_across(sl.nx), tiles_y = tiles_across(sl.ny);
    // (the nine marks read together -- a neighbour that does not exist reads the tile's own mark -- not one after the other behind
    // `any ||`: up to nine dependent round trips at the head of a tile that turns out to be out of reach)
    const unsigned char* __restrict__ marks = s.bf_tile_charge;
    unsigned char m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        int ux = tx + k % 3 - 1, uy = ty + k / 3 - 1;
        if (ux < 0 || uy < 0 || ux >= tiles_x || uy >= tiles_y) { ux = tx; uy = ty; }
        m[k] = marks[cell_index(sl, ux * UT, uy * UT)];
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) any = any || (m[k] == (unsigned char)tag);
    return !any;
}

__global__ __launch_bounds__(256) void k_update_distortions(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                            const int64_t* __restrict__ tile_prefix,
                                                            unsigned char* __restrict__ changed, unsigned int tag)
{
    __shared__ double tile[UH * UH];
    const ims_sensor_t& s = *sp;
    // block -> (slot, tile)
    const int64_t b = blockIdx.x;
    const int lo = find_slot(tile_prefix, n_slots, b);
    const ims_bf_slot_t bs = s.bf_slots[first_slot + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int t = (int)(b - tile_prefix[lo]);
    const int tx0 = (t % tiles_x) * UT, ty0 = (t / tiles_x) * UT;
    if (tile_out_of_reach(s, sl, tx0 / UT, ty0 / UT, tag)) return;
    const int q = s.qdist;
    const int hw = UT + 2 * q + 1;                 // halo tile edge
    const int sx0 = tx0 - (q + 1), sy0 = ty0 - (q + 1);
    for (int e = threadIdx.x; e < hw * hw; e += 256) {
        const int hx = e % hw, hy = e / hw;
        const int si = sx0 + hx, sj = sy0 + hy;
        double v = 0.0;
        if (si >= 0 && si < sl.nx && sj >= 0 && sj < sl.ny) v = s.bf_delta[cell_index(sl, si, sj)];
        tile[hy * hw + hx] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x % UT, ly = threadIdx.x / UT;
    const int i = tx0 + lx, j = ty0 + ly;
    if (i > sl.nx || j > sl.ny) return;
    const int nV = s.num_vertices, npo = 2 * nV + 2, nv = 4 * nV + 4;
    const int cx = (s.nx - 1) / 2, cy = (s.ny - 1) / 2;
    const int64_t c = cell_index(sl, i, j);
    double* pts = s.bf_boundary + c * npo * 2;
    bool any = false;
    for (int dj = -q; dj <= q + 1; ++dj) {
        const int sj = j - dj;
        if (sj < 0 || sj >= sl.ny) continue;
        for (int di = -q; di <= q + 1; ++di) {
            const int si = i - di;
            if (si < 0 || si >= sl.nx) continue;
            const double charge = tile[(sj - sy0) * hw + (si - sx0)];
            if (charge == 0.0) continue;
            any = true;
            const double w = ddiv(charge, s.num_elec);
            // An edge takes the table entry of the pixel it is the bottom row / left edge of.  On the extra row / column of a qdist
            // that reaches the stamp's rim (4 with the 9 x 9 files) that pixel is not tabulated: the edge is then the top row /
            // right edge of the stamp's last pixel, read from its end (top row) or in place (right edge, bottom to top).
            const bool row_out = dj + cy >= s.ny, col_out = di + cx >= s.nx;
            for (int n = 0; n < npo; ++n) {
                if (n <= nV + 1 && di == q + 1) continue;
                if (n > nV + 1 && dj == q + 1) continue;
                const bool bottom = n <= nV + 1;
                const int ti = di + cx - ((!bottom && col_out) ? 1 : 0), tj = dj + cy - ((bottom && row_out) ? 1 : 0);
                const int vtx = bottom ? (row_out ? 3 * nV + 3 - n : n) : (col_out ? n : owned_to_vertex(nV, n));
                const double* dist = s.distortions + ((int64_t)ti * s.ny + tj) * nv * 2;
                pts[2 * n] = fma(dist[2 * vtx], w, pts[2 * n]);
                pts[2 * n + 1] = fma(dist[2 * vtx + 1], w, pts[2 * n + 1]);
            }
        }
    }
    changed[c] = any ? 1 : 0;
    if (any && tag != 0u && s.bf_tile_changed != nullptr) s.bf_tile_changed[cell_index(sl, tx0, ty0)] = (unsigned char)tag;
}

// LDS of one q3 tile update: scaled charges of the halo, per-row occupancy bitmaps, displacement table
template <int NV>
struct UpdateLds {
    static constexpr int Q = 3, HW = UT + 2 * Q + 1, NPO = 2 * NV + 2;
    double wt[HW * HW];
    double dl[8 * 8 * NPO * 2];           // [dj+Q][di+Q][owned point][x,y]
    unsigned int occ[HW];
    int any_charge;
};

template <int NV>
__device__ __forceinline__ void load_displacements(const ims_sensor_t& s, UpdateLds<NV>& L)
{
    constexpr int Q = 3, NPO = 2 * NV + 2, NVV = 4 * NV + 4;
    const int cx = (s.nx - 1) / 2, cy = (s.ny - 1) / 2;
    for (int e = threadIdx.x; e < 8 * 8 * NPO * 2; e += 256) {
        const int comp = e & 1, n = (e >> 1) % NPO, cell = (e >> 1) / NPO;
        const int di = (cell & 7) - Q, dj = (cell >> 3) - Q;
        const int vtx = owned_to_vertex(NV, n);
        L.dl[e] = s.distortions[(((int64_t)(di + cx) * s.ny + (dj + cy)) * NVV + vtx) * 2 + comp];
    }
}

// Silicon::updatePixelDistortions for the 16x16 owner cells of tile (tx0, ty0) of one slot (qdist 3).
// dl_loaded: the displacement table is already in L.dl (persistent kernels load it once).  Returns, per thread,
// whether its cell moved; `tile_moved` is set when any cell of the tile did.
// DlPtr: the type of the global table's pointer -- a kernel's own restrict-qualified argument, or (joint launches, where the
// pointer comes out of an argument block and carries no aliasing information) a pointer into the constant address space, whose
// loads at uniform addresses are scalar loads by definition.
typedef const double __attribute__((address_space(4))) * ConstTable;

template <int NV, bool GLOBAL_DL = false, class DlPtr = const double*>
__device__ __forceinline__ void update_tile_q3(const ims_sensor_t& s, const SlotView& sl, int tx0, int ty0,
                                               unsigned char* __restrict__ changed, UpdateLds<NV>& L, bool dl_loaded,
                                               unsigned int tag, DlPtr __restrict__ dl_global = nullptr)
{
    constexpr int Q = 3, HW = UT + 2 * Q + 1, NPO = 2 * NV + 2;
    const int sx0 = tx0 - (Q + 1), sy0 = ty0 - (Q + 1);
    PROBE(9);
    if (threadIdx.x < HW) L.occ[threadIdx.x] = 0u;
    if (threadIdx.x == 0) L.any_charge = 0;
    // the halo's 529 cells, up to three per thread, requested TOGETHER: as a rolled loop (load, wait, scale, store, next) they were three
    // dependent memory round trips at the head of every tile -- behind a kernel boundary ~1.5 us each under load (round 6)
    constexpr int HE = (HW * HW + 255) / 256;
    double charge[HE];
    const double num_elec = s.num_elec;
#pragma unroll
    for (int u = 0; u < HE; ++u) {
        const int e = (int)threadIdx.x + 256 * u;
        const int hx = e % HW, hy = e / HW;
        const int si = sx0 + hx, sj = sy0 + hy;
        const bool in = e < HW * HW && si >= 0 && si < sl.nx && sj >= 0 && sj < sl.ny;
        charge[u] = in ? (double)s.bf_delta[cell_index(sl, si, sj)] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HE; ++u) {
        const int e = (int)threadIdx.x + 256 * u;
        if (e < HW * HW) {
            double w = 0.0;
            if (charge[u] != 0.0) { w = ddiv(charge[u], num_elec); atomicOr(&L.occ[e / HW], 1u << (e % HW)); L.any_charge = 1; }
            L.wt[e] = w;
        }
    }
    __syncthreads();
    PROBE(10);
    const int lx = threadIdx.x % UT, ly = threadIdx.x / UT;
    const int i = tx0 + lx, j = ty0 + ly;
    if (!L.any_charge) {                     // nothing landed near this tile: nothing moves
        if (i <= sl.nx && j <= sl.ny) changed[cell_index(sl, i, j)] = 0;
        return;
    }
    if (!GLOBAL_DL && !dl_loaded) {
        load_displacements<NV>(s, L);
        __syncthreads();
    }
    PROBE(11);
    if (i > sl.nx || j > sl.ny) return;
    // 64-bit window: byte a <-> dj = -Q + a (row hy = ly + 2Q + 1 - a); inside a byte bit bb <-> di = -Q + bb
    // (column hx = lx + 2Q + 1 - bb), i.e. the row bitmap reversed.
    unsigned long long mask = 0ull;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const unsigned int row = (L.occ[ly + 2 * Q + 1 - a] >> lx) & 0xFFu;
        const unsigned int rev = __brev(row) >> 24;
        mask |= (unsigned long long)rev << (8 * a);
    }
    const int64_t c = cell_index(sl, i, j);
    changed[c] = mask ? 1 : 0;
    if (!mask) return;
    if (tag != 0u && s.bf_tile_changed != nullptr) s.bf_tile_changed[cell_index(sl, tx0, ty0)] = (unsigned char)tag;
    double* pts = s.bf_boundary + c * NPO * 2;
    double acc[NPO * 2];
#pragma unroll
    for (int n = 0; n < NPO * 2; ++n) acc[n] = pts[n];
    PROBE(12);
    // The 8 x 8 source window with STATIC offsets, in the spec's order (dj ascending, then di ascending).  A bright
    // star's region is a few hundred tiles, so a SIMD holds ONE wavefront and nothing hides latency: the bit-walking loop
    // (address of the displacement row from the next set bit) waited ~850 cycles per neighbour.  Here every row of the
    // window is straight-line code: the displacement rows sit at compile-time addresses (SGPRs through the scalar cache
    // with the global table, LDS broadcasts otherwise), the scaled charge w of a neighbour without charge is exactly 0
    // and fma(d, +0, acc) leaves acc unchanged bit for bit (acc is never -0: the initial points are +0 / positive plus a
    // tree-ring shift, and an exact cancellation rounds to +0), so no lane needs a branch; a row of the window that no
    // lane of the wavefront needs is skipped as a whole.
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const unsigned int rowbits = (unsigned int)(mask >> (8 * a)) & 0xFFu;
        if (__builtin_amdgcn_ballot_w64(rowbits != 0u) == 0ull) continue;
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
            const double w = L.wt[(ly + 2 * Q + 1 - a) * HW + (lx + 2 * Q + 1 - bb)];
            // GLOBAL_DL: the row comes through the scalar cache into SGPRs (uniform, read-only table of the launch)
            auto row = [&](auto d) {
                if (bb != 7) {                     // not the extra column: bottom-row points
#pragma unroll
                    for (int n = 0; n <= NV + 1; ++n) {
                        acc[2 * n] = fma(d[2 * n], w, acc[2 * n]);
                        acc[2 * n + 1] = fma(d[2 * n + 1], w, acc[2 * n + 1]);
                    }
                }
                if (a != 7) {                      // not the extra row: left-edge points
#pragma unroll
                    for (int n = NV + 2; n < NPO; ++n) {
                        acc[2 * n] = fma(d[2 * n], w, acc[2 * n]);
                        acc[2 * n + 1] = fma(d[2 * n + 1], w, acc[2 * n + 1]);
                    }
                }
            };
            if constexpr (GLOBAL_DL) row(dl_global + (a * 8 + bb) * NPO * 2);
            else row((const double*)L.dl + (a * 8 + bb) * NPO * 2);
        }
    }
    PROBE(13);
#pragma unroll
    for (int n = 0; n < NPO * 2; ++n) pts[n] = acc[n];
    PROBE(14);
}

// acc = fma(d of lane SEL of this lane's row of 16, w, acc): the DPP form of v_fmac_f64 (gfx90a and later accept
// row_newbcast on the 64-bit ALU).  The operand that is uniform over the wavefront -- an entry of the displacement table --
// sits in ONE lane of every row of a VGPR pair and is broadcast by the instruction itself: no scalar load, no LDS read and
// no wait between the FMAs.  All 64 lanes must be active (the source lane is read through EXEC).
__device__ __forceinline__ void fmac_bcast(int sel, double& acc, double d, double w)
{
#define IMS_FB(n) case n: asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #n " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(d), "v"(w)); break;
    switch (sel) {
        IMS_FB(0) IMS_FB(1) IMS_FB(2) IMS_FB(3) IMS_FB(4) IMS_FB(5) IMS_FB(6) IMS_FB(7)
        IMS_FB(8) IMS_FB(9) IMS_FB(10) IMS_FB(11) IMS_FB(12) IMS_FB(13) IMS_FB(14) IMS_FB(15)
    }
#undef IMS_FB
}

// update_tile_q3 with the displacement table delivered by DPP broadcasts.  In the form above a tap costs two scalar
// loads, a wait for them and twenty FMAs on SGPR operands: the 102 SGPRs hold two taps at most, so nothing is fetched ahead
// and a cell's 64 taps are 128 scalar-cache round trips -- 10.8 of the kernel's 14 us for a star's core tile.  Here the
// table is staged in LDS once per workgroup (beside the charge halo, one round trip for both), a row of the window (8 taps
// x 2 NPO values) is read as NPO VGPR pairs, lane l holding entry 16 r + (l & 15), and every FMA names the lane it wants.
// Same operands, same order, same bits.  Lanes without a cell or without charge in their window run along (their w are
// +0, which leaves acc unchanged bit for bit) because a broadcast reads its source lane through EXEC.
// early_table: the table's loads are issued before the halo's (one round trip for both: a star's few tiles, where the latency of
// a round counts); otherwise only the tiles that found charge fetch it (a wide launch is mostly tiles without: 10 KB each).
template <int NV>
__device__ __forceinline__ void update_tile_q3_dpp(const ims_sensor_t& s, const SlotView& sl, int tx0, int ty0,
                                                   unsigned char* __restrict__ changed, UpdateLds<NV>& L, unsigned int tag,
                                                   const double* __restrict__ dl_global, bool early_table)
{
    constexpr int Q = 3, HW = UT + 2 * Q + 1, NPO = 2 * NV + 2, NPT = 2 * NPO;
    const int sx0 = tx0 - (Q + 1), sy0 = ty0 - (Q + 1);
    if (threadIdx.x < HW) L.occ[threadIdx.x] = 0u;
    if (threadIdx.x == 0) L.any_charge = 0;
    // the table first: its loads fly while the halo is gathered
    constexpr int DLN = 8 * 8 * NPT, DLP = (DLN + 255) / 256;
    double dreg[DLP];
    if (early_table) {
#pragma unroll
        for (int u = 0; u < DLP; ++u) {
            const int e = threadIdx.x + 256 * u;
            dreg[u] = (e < DLN) ? dl_global[e] : 0.0;
        }
    }
    constexpr int HE = (HW * HW + 255) / 256;
    double charge[HE];                               // (requested together, as in update_tile_q3)
    const double num_elec = s.num_elec;
#pragma unroll
    for (int u = 0; u < HE; ++u) {
        const int e = (int)threadIdx.x + 256 * u;
        const int hx = e % HW, hy = e / HW;
        const int si = sx0 + hx, sj = sy0 + hy;
        const bool in = e < HW * HW && si >= 0 && si < sl.nx && sj >= 0 && sj < sl.ny;
        charge[u] = in ? (double)s.bf_delta[cell_index(sl, si, sj)] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HE; ++u) {
        const int e = (int)threadIdx.x + 256 * u;
        if (e < HW * HW) {
            double w = 0.0;
            if (charge[u] != 0.0) { w = ddiv(charge[u], num_elec); atomicOr(&L.occ[e / HW], 1u << (e % HW)); L.any_charge = 1; }
            L.wt[e] = w;
        }
    }
    if (early_table) {
#pragma unroll
        for (int u = 0; u < DLP; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < DLN) L.dl[e] = dreg[u];
        }
    }
    __syncthreads();
    const int lx = threadIdx.x % UT, ly = threadIdx.x / UT;
    const int i = tx0 + lx, j = ty0 + ly;
    const bool cell = (i <= sl.nx && j <= sl.ny);
    if (!L.any_charge) {                     // nothing landed near this tile: nothing moves
        if (cell) changed[cell_index(sl, i, j)] = 0;
        return;
    }
    if (!early_table) {
        for (int e = threadIdx.x; e < DLN; e += 256) L.dl[e] = dl_global[e];
        __syncthreads();
    }
    unsigned long long mask = 0ull;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const unsigned int row = (L.occ[ly + 2 * Q + 1 - a] >> lx) & 0xFFu;
        const unsigned int rev = __brev(row) >> 24;
        mask |= (unsigned long long)rev << (8 * a);
    }
    if (!cell) mask = 0ull;
    const int64_t c = cell ? cell_index(sl, i, j) : sl.offset;
    if (cell) changed[c] = mask ? 1 : 0;
    if (mask && tag != 0u && s.bf_tile_changed != nullptr) s.bf_tile_changed[cell_index(sl, tx0, ty0)] = (unsigned char)tag;
    double* pts = s.bf_boundary + c * NPT;
    double acc[NPT];
#pragma unroll
    for (int n = 0; n < NPT; ++n) acc[n] = mask ? pts[n] : 0.0;
    const int l16 = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const unsigned int rowbits = (unsigned int)(mask >> (8 * a)) & 0xFFu;
        if (__builtin_amdgcn_ballot_w64(rowbits != 0u) == 0ull) continue;
        double d[NPO], w[8];
#pragma unroll
        for (int r = 0; r < NPO; ++r) d[r] = L.dl[a * 8 * NPT + r * 16 + l16];
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
            const double ww = L.wt[(ly + 2 * Q + 1 - a) * HW + (lx + 2 * Q + 1 - bb)];
            w[bb] = mask ? ww : 0.0;
        }
#pragma unroll
        for (int bb = 0; bb < 8; ++bb) {
            if (__builtin_amdgcn_ballot_w64(w[bb] != 0.0) == 0ull) continue;       // a tap no lane of the wavefront has charge under
#pragma unroll
            for (int n2 = 0; n2 < NPT; ++n2) {
                const bool bottom = n2 < 2 * (NV + 2);
                if (bottom ? (bb == 7) : (a == 7)) continue;                    // the extra column / row of the window
                const int v = bb * NPT + n2;
                fmac_bcast(v & 15, acc[n2], d[v >> 4], w[bb]);
            }
        }
    }
    if (mask) {
#pragma unroll
        for (int n = 0; n < NPT; ++n) pts[n] = acc[n];
    }
}

// Fast path for qdist == 3 (the GalSim default): the 8x8 source window of a cell is a 64-bit
// occupancy mask cut out of per-row LDS bitmaps, so a lane only iterates over its OWN charged
// neighbours (in the spec's order: dj ascending, then di ascending) instead of testing all 64.
// Sparse stamp wings cost max-over-lanes(nnz) iterations per wave; the dense core stays dense.
// Boundary points are accumulated in registers (NV is a template parameter) and the displacement
// table and the scaled charges w = delta / num_elec live in LDS.
template <int NV, bool DPP = false>
__global__ __launch_bounds__(256) void k_update_distortions_q3(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                               const int64_t* __restrict__ tile_prefix,
                                                               unsigned char* __restrict__ changed, unsigned int tag,
                                                               const double* __restrict__ dl_global)
{
    __shared__ UpdateLds<NV> L;
    PROBE(8);
    const ims_sensor_t& s = *sp;
    const int64_t b = blockIdx.x;
    const int lo = find_slot(tile_prefix, n_slots, b);
    const ims_bf_slot_t bs = s.bf_slots[first_slot + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int t = (int)(b - tile_prefix[lo]);
    const int tx0 = (t % tiles_x) * UT, ty0 = (t / tiles_x) * UT;
    if (tile_out_of_reach(s, sl, tx0 / UT, ty0 / UT, tag)) return;
#ifdef IMS_UPD_FORCE_LDS
    dl_global = nullptr;
#endif
    if (DPP) update_tile_q3_dpp<NV>(s, sl, tx0, ty0, changed, L, tag, dl_global, gridDim.x <= 64u);
    else if (dl_global != nullptr) update_tile_q3<NV, true>(s, sl, tx0, ty0, changed, L, false, tag, dl_global);
    else update_tile_q3<NV, false>(s, sl, tx0, ty0, changed, L, false, tag);
}

// the update of several CCDs' regions in one launch (k_accumulate_round_j): per chain the sensor, its slots, tile prefix and flags
struct JointUpd {                           // constant over the rounds: device memory
    const ims_sensor_t* sp[IMS_JOINT_MAX];
    const int64_t* tile_prefix[IMS_JOINT_MAX];
    unsigned char* changed[IMS_JOINT_MAX];
    const double* dl[IMS_JOINT_MAX];
    int32_t first_slot[IMS_JOINT_MAX];
};

struct JointTables { JointAcc acc; JointUpd upd; };

// the tables of one joint run go to device memory as the by-value arguments of small launches, eight chains at a time (a kernel's
// arguments are limited to 4 KB): stream-ordered, no staging
constexpr int JOINT_CHUNK = 8;
struct JointChunk {
    RoundArgs a[JOINT_CHUNK];
    const int64_t* pool_start[JOINT_CHUNK];
    const ims_sensor_t* sp[JOINT_CHUNK];
    const int64_t* tile_prefix[JOINT_CHUNK];
    unsigned char* changed[JOINT_CHUNK];
    const double* dl[JOINT_CHUNK];
    unsigned int* words[JOINT_CHUNK];
    int32_t first_slot[JOINT_CHUNK];
};

__global__ __launch_bounds__(64) void k_store_joint_tables(const JointChunk C, JointTables* __restrict__ dst, int k0)
{
    const int k = (int)threadIdx.x;
    if (k >= JOINT_CHUNK) return;
    dst->acc.a[k0 + k] = C.a[k];
    dst->acc.pool_start[k0 + k] = C.pool_start[k];
    dst->upd.sp[k0 + k] = C.sp[k];
    dst->upd.tile_prefix[k0 + k] = C.tile_prefix[k];
    dst->upd.changed[k0 + k] = C.changed[k];
    dst->upd.dl[k0 + k] = C.dl[k];
    dst->upd.first_slot[k0 + k] = C.first_slot[k];
    dst->acc.tile_prefix[k0 + k] = C.tile_prefix[k];
    dst->acc.words[k0 + k] = C.words[k];
    dst->acc.first_slot[k0 + k] = C.first_slot[k];
}

// (the body as a function of restrict-qualified pointers: loaded from the argument block they would carry no aliasing
// information, and the SGPR form of the update then needs 122 registers instead of 72)
template <int NV, bool DPP>
__device__ __forceinline__ void update_block_q3(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                const int64_t* __restrict__ tile_prefix, unsigned char* __restrict__ changed,
                                                unsigned int tag, const double* __restrict__ dl_global, int64_t b, bool small,
                                                UpdateLds<NV>& L)
{
    const ims_sensor_t& s = *sp;
    const int lo = find_slot(tile_prefix, n_slots, b);
    const ims_bf_slot_t bs = s.bf_slots[first_slot + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int t = (int)(b - tile_prefix[lo]);
    const int tx0 = (t % tiles_x) * UT, ty0 = (t / tiles_x) * UT;
    if (tile_out_of_reach(s, sl, tx0 / UT, ty0 / UT, tag)) return;
    if (DPP) update_tile_q3_dpp<NV>(s, sl, tx0, ty0, changed, L, tag, dl_global, small);
    else if (dl_global != nullptr) update_tile_q3<NV, true, ConstTable>(s, sl, tx0, ty0, changed, L, false, tag, (ConstTable)(uintptr_t)dl_global);
    else update_tile_q3<NV, false>(s, sl, tx0, ty0, changed, L, false, tag);
}

template <int NV, bool DPP = false>
__global__ __launch_bounds__(256) void k_update_distortions_q3_j(const JointUpd* __restrict__ U, const JointRound* __restrict__ R,
                                                                 unsigned int tag)
{
    __shared__ UpdateLds<NV> L;
    int bb = (int)blockIdx.x;
    const int c = joint_chain(&R->eu, bb);
    update_block_q3<NV, DPP>(U->sp[c], U->first_slot[c], joint_entry(&R->ns, c), U->tile_prefix[c], U->changed[c], tag, U->dl[c], (int64_t)bb,
                             gridDim.x <= 64u, L);
}


// bounds of the pixels whose polygon moved (own cell, right cell or upper cell changed); one 16x16
// tile of owner cells per workgroup, same grid as the update kernel.  With a tag, tiles that saw
// neither charge nor movement (own, right and upper tile) leave after three byte loads.
// NV > 0: the owned points of the cell and of its right / upper neighbours are fetched with independent loads into
// registers and the vertex loop is unrolled (the generic loop issues one dependent load per vertex: 12 us per wave).
// fold_image: the f64 image of which this slot is the pixel grid (row length sl.nx): the consumed delta charge is added to it --
// Silicon's `target += delta` at a recalculation (deposits of ims_render_params_t.track_static_delta 2 went to the delta image only)
template <int NV>
__device__ __forceinline__ void refresh_tile(const ims_sensor_t& s, const SlotView& sl, int tx, int ty, bool own, bool right,
                                             bool up, bool charged, const unsigned char* __restrict__ changed,
                                             double* __restrict__ fold_image = nullptr)
{
    const int lx = threadIdx.x % UT, ly = threadIdx.x / UT;
    const int i = tx * UT + lx, j = ty * UT + ly;
    if (i > sl.nx || j > sl.ny) return;
    const int64_t c = cell_index(sl, i, j);
    if (charged) {                            // the update has consumed the delta charge
        if (fold_image != nullptr && i < sl.nx && j < sl.ny) {
            const double d = s.bf_delta[c];
            if (d != 0.0) fold_image[(int64_t)j * sl.nx + i] += d;
        }
        s.bf_delta[c] = 0.0;
    }
    if (i >= sl.nx || j >= sl.ny) return;
    // per-cell flags are only meaningful in tiles the update worked on this round
    // (the three bytes are read whether or not their tile's flag asks for them -- (i + 1, j) and (i, j + 1) are owner cells of the
    // region, i < nx and j < ny here -- so that they are ONE round trip, not up to three behind short-circuit tests)
    const unsigned char c_own = changed[c], c_right = changed[cell_index(sl, i + 1, j)], c_up = changed[cell_index(sl, i, j + 1)];
    const bool f_own = own && c_own;
    const bool f_right = ((lx + 1 < UT) ? own : right) && c_right;
    const bool f_up = ((ly + 1 < UT) ? own : up) && c_up;
    if (!(f_own || f_right || f_up)) return;
    const int nV = (NV > 0) ? NV : s.num_vertices, nv = 4 * nV + 4;
    double ixmin = 0.0, ixmax = 1.0, iymin = 0.0, iymax = 1.0;
    double oxmin = 0.0, oxmax = 1.0, oymin = 0.0, oymax = 1.0;
    double v0x = 0.0;
    if (NV > 0) {
        constexpr int NPO = 2 * NV + 2;
        constexpr int NVX = (NV > 0) ? NV : 1;
        double2 ownp[(NV > 0) ? NPO : 1], rgt[NVX], upp[(NV > 0) ? NV + 2 : 1];
        const double2* po = (const double2*)(s.bf_boundary + c * NPO * 2);
        const double2* pr = (const double2*)(s.bf_boundary + cell_index(sl, i + 1, j) * NPO * 2);
        const double2* pu = (const double2*)(s.bf_boundary + cell_index(sl, i, j + 1) * NPO * 2);
#pragma unroll
        for (int q = 0; q < NPO; ++q) ownp[q] = po[q];
#pragma unroll
        for (int m = 0; m < NV; ++m) rgt[m] = pr[NV + 2 + m];
#pragma unroll
        for (int q = 0; q < NV + 2; ++q) upp[q] = pu[q];
#pragma unroll
        for (int k = 0; k < 4 * NV + 4; ++k) {
            double vx, vy;
            if (k <= NV + 1) { vx = ownp[k].x; vy = ownp[k].y; }
            else if (k <= 2 * NV + 1) { vx = rgt[k - NV - 2].x + 1.0; vy = rgt[k - NV - 2].y; }
            else if (k <= 3 * NV + 3) { vx = upp[NV + 1 - (k - 2 * NV - 2)].x; vy = upp[NV + 1 - (k - 2 * NV - 2)].y + 1.0; }
            else { vx = ownp[NV + 2 + (NV - 1 - (k - 3 * NV - 4))].x; vy = ownp[NV + 2 + (NV - 1 - (k - 3 * NV - 4))].y; }
            if (k == 0) v0x = vx;
            if (vx < oxmin) oxmin = vx;
            if (vx > oxmax) oxmax = vx;
            if (vy < oymin) oymin = vy;
            if (vy > oymax) oymax = vy;
            if (k <= NV + 1) { if (vy > iymin) iymin = vy; }
            if (k >= NV + 1 && k <= 2 * NV + 2) { if (vx < ixmax) ixmax = vx; }
            if (k >= 2 * NV + 2 && k <= 3 * NV + 3) { if (vy < iymax) iymax = vy; }
            if (k >= 3 * NV + 3) { if (vx > ixmin) ixmin = vx; }
        }
    } else {
        for (int k = 0; k < nv; ++k) {
            double vx, vy;
            polygon_vertex(s, sl, i, j, k, 1.0, vx, vy);
            if (k == 0) v0x = vx;
            if (vx < oxmin) oxmin = vx;
            if (vx > oxmax) oxmax = vx;
            if (vy < oymin) oymin = vy;
            if (vy > oymax) oymax = vy;
            if (k <= nV + 1) { if (vy > iymin) iymin = vy; }
            if (k >= nV + 1 && k <= 2 * nV + 2) { if (vx < ixmax) ixmax = vx; }
            if (k >= 2 * nV + 2 && k <= 3 * nV + 3) { if (vy < iymax) iymax = vy; }
            if (k >= 3 * nV + 3) { if (vx > ixmin) ixmin = vx; }
        }
    }
    if (v0x > ixmin) ixmin = v0x;
    double* bb = s.bf_bounds + c * 8;
    bb[0] = ixmin; bb[1] = ixmax; bb[2] = iymin; bb[3] = iymax;
    bb[4] = oxmin; bb[5] = oxmax; bb[6] = oymin; bb[7] = oymax;
}

// which marks carry this round's tag: the tile's own, its right / upper neighbour's `changed` mark, its charge mark; false: none (nothing to refresh)
struct TileAt { SlotView sl; int tx, ty, tiles_x; };   // (the tagged kernels name one in a block: as plain arguments k_refresh_changed_j takes 32 SGPRs for 30)
__device__ __forceinline__ bool refresh_flags(const ims_sensor_t& s, const TileAt& T, unsigned int tag, bool& own, bool& right, bool& up, bool& charged)
{
    const SlotView& sl = T.sl; const int tx = T.tx, ty = T.ty, tiles_x = T.tiles_x;
    const unsigned char tg = (unsigned char)tag;
    // (the four bytes in ONE round trip: the right / upper tile's at the tile's own address where there is none)
    const bool has_r = tx + 1 < tiles_x, has_u = ty + 1 < tiles_across(sl.ny);
    const unsigned char t_own = s.bf_tile_changed[cell_index(sl, tx * UT, ty * UT)],
                        t_right = s.bf_tile_changed[cell_index(sl, (has_r ? tx + 1 : tx) * UT, ty * UT)],
                        t_up = s.bf_tile_changed[cell_index(sl, tx * UT, (has_u ? ty + 1 : ty) * UT)],
                        t_charge = s.bf_tile_charge[cell_index(sl, tx * UT, ty * UT)];
    own = t_own == tg; right = has_r && t_right == tg; up = has_u && t_up == tg; charged = t_charge == tg;
    return own || right || up || charged;
}

template <int NV>
__global__ __launch_bounds__(256) void k_refresh_changed(const ims_sensor_t* __restrict__ sp, int first_slot, int n_slots,
                                                         const int64_t* __restrict__ tile_prefix,
                                                         const unsigned char* __restrict__ changed, unsigned int tag,
                                                         double* __restrict__ fold_image)
{
    PROBE(16);
    const ims_sensor_t& s = *sp;
    const int64_t b = blockIdx.x;
    const int lo = find_slot(tile_prefix, n_slots, b);
    const ims_bf_slot_t bs = s.bf_slots[first_slot + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int t = (int)(b - tile_prefix[lo]);
    const int tx = t % tiles_x, ty = t / tiles_x;
    const bool flags = (tag != 0u) && s.bf_tile_charge != nullptr && s.bf_tile_changed != nullptr;
    bool own = true, right = true, up = true, charged = true;
    if (flags) {
        const TileAt T = { sl, tx, ty, tiles_x }; if (!refresh_flags(s, T, tag, own, right, up, charged)) return;
    }
    PROBE(17);
    refresh_tile<NV>(s, sl, tx, ty, own, right, up, charged, changed, fold_image);
    PROBE(18);
}

template <int NV>
__global__ __launch_bounds__(256) void k_refresh_changed_j(const JointUpd* __restrict__ U, const JointRound* __restrict__ R,
                                                           unsigned int tag)
{
    int bb = (int)blockIdx.x;
    const int c = joint_chain(&R->eu, bb);
    const ims_sensor_t& s = *U->sp[c];
    const int64_t* __restrict__ tile_prefix = U->tile_prefix[c];
    const unsigned char* changed = U->changed[c];
    const int64_t b = bb;
    const int lo = find_slot(tile_prefix, joint_entry(&R->ns, c), b);
    const ims_bf_slot_t bs = s.bf_slots[U->first_slot[c] + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int t = (int)(b - tile_prefix[lo]);
    const int tx = t % tiles_x, ty = t / tiles_x;
    const bool flags = (tag != 0u) && s.bf_tile_charge != nullptr && s.bf_tile_changed != nullptr;
    bool own = true, right = true, up = true, charged = true;
    if (flags) {
        const TileAt T = { sl, tx, ty, tiles_x }; if (!refresh_flags(s, T, tag, own, right, up, charged)) return;
    }
    refresh_tile<NV>(s, sl, tx, ty, own, right, up, charged, changed);
}

// ---- joint rounds over the ACTIVE tiles only ----
// A round's update and refresh launches held one workgroup per 16 x 16 tile of every region of every chain -- 24 000 workgroups
// for the brightest stars of eight CCDs (678 x 678-pixel stamps: 1 849 tiles each), of which a few thousand find charge within
// reach; the rest leave at once, but their dispatch is what the launch costs (4 ns per workgroup alone, twice that beside the
// photon kernels: 50 - 90 us of a 110-us round).  Here one thread per tile reads the charge marks the pixel search left
// (ims_sensor_t.bf_tile_charge, this round's tag) and appends the tiles within reach to a list -- and those whose bounds can
// change (the tile itself, its right or its upper neighbour within reach) to a second one; the update and refresh launches
// then hold a fraction of the workgroups and walk the lists.  Same decisions as the tagged kernels, tile by tile: same bits.
struct JointLists {
    unsigned long long* upd;            // entries: pack_tile_entry
    unsigned long long* ref;
    int* count;                         // [parity][2]: entries of upd / ref
};

// fine: a tile that passes the test on the tile marks is looked at block by block (mark_tile_charge: 4 x 4 pixels).  The update
// of tile [tx0, tx0 + 15]^2 reads the delta charge of [tx0 - 4, tx0 + 18]^2 (update_tile_q3: Q = 3) and changes nothing without
// charge there; those are the blocks -1 .. 4 of the tile in x and y.  The bounds of the tile's pixels also hang on the first
// column of the right tile and the first row of the upper one, which move with charge in [tx0 + 12, tx0 + 19] x [ty0 - 4, ty0 + 18]
// (and transposed): blocks 3 .. 4, inside the same window.  So ONE test decides both lists, and a lone electron in the wings of
// a star lists the one or two tiles within four pixels of it instead of nine.  Tiles that are listed do what they did; tiles
// that are no longer listed would have found no charge in their halo and left (update_tile_q3: !any_charge) -- their `changed`
// bytes stay as they are, which can make the refresh of a LATER round recompute bounds that did not move (same bits).
__global__ __launch_bounds__(256) void k_build_active_j(const JointUpd* __restrict__ U, const JointRound* __restrict__ R,
                                                        unsigned int tag, const JointLists Ls, int parity, int fine)
{
    int bb = (int)blockIdx.x;
    const int c = joint_chain(&R->ewg, bb);
    const ims_sensor_t& s = *U->sp[c];
    const int64_t* __restrict__ tile_prefix = U->tile_prefix[c];
    const int n_tiles = joint_entry(&R->tof, c), ns = joint_entry(&R->ns, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) { Ls.count[2 * (parity ^ 1)] = 0; Ls.count[2 * (parity ^ 1) + 1] = 0; }   // the next round's
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)bb * 256 + threadIdx.x;
    bool todo = g < n_tiles;
    int my_lo = 0, my_t = 0;
    // slot of every lane's tile: the wavefront resolves one slot per turn (find_slot wants all 64 lanes)
    unsigned long long pending = __builtin_amdgcn_ballot_w64(todo);
    while (pending != 0ull) {
        const int src = __builtin_ctzll(pending);
        const int64_t gf = __shfl(g, src, 64);
        const int lo = find_slot(tile_prefix, ns, gf);
        const int64_t p0 = tile_prefix[lo], p1 = tile_prefix[lo + 1];
        if (todo && g >= p0 && g < p1) { my_lo = lo; my_t = (int)(g - p0); todo = false; }
        pending = __builtin_amdgcn_ballot_w64(todo);
    }
    bool in_reach = false, bounds = false;
    if (g < n_tiles) {
        const ims_bf_slot_t bs = s.bf_slots[U->first_slot[c] + my_lo];
        const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
        const int tiles_x = tiles_across(sl.nx), tiles_y = tiles_across(sl.ny);
        const int tx = my_t % tiles_x, ty = my_t / tiles_x;
        const unsigned char tg = (unsigned char)tag;
        // charge marks of the 4 x 4 window (-1 .. 2)^2 around the tile, as bits
        unsigned int m = 0u;
#pragma unroll
        for (int dy = -1; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 2; ++dx) {
                const int ux = tx + dx, uy = ty + dy;
                if (ux < 0 || uy < 0 || ux >= tiles_x || uy >= tiles_y) continue;
                if (s.bf_tile_charge[cell_index(sl, ux * UT, uy * UT)] == tg) m |= 1u << ((dy + 1) * 4 + (dx + 1));
            }
        // 3 x 3 windows around the tile, its right and its upper neighbour (bit = row * 4 + column of the 4 x 4 window)
        const unsigned int own_w = 0x0777u, right_w = 0x0EEEu, up_w = 0x7770u;
        in_reach = (m & own_w) != 0u;
        const bool right_in = tx + 1 < tiles_x && (m & right_w) != 0u;
        const bool up_in = ty + 1 < tiles_y && (m & up_w) != 0u;
        bounds = in_reach || right_in || up_in;
        if (fine && bounds) {
            // charge in the tile itself is in reach; otherwise only the blocks of the marked neighbours that touch this tile are
            // looked at (an edge neighbour's four, a corner neighbour's one): 1 .. 20 bytes instead of the window's 36
            bool any = (m & (1u << 5)) != 0u;
            if (!any) {
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dx == 0 && dy == 0) || !(m & (1u << ((dy + 1) * 4 + (dx + 1))))) continue;
                        const int bx0 = dx < 0 ? -1 : (dx > 0 ? 4 : 0), bx1 = dx < 0 ? -1 : (dx > 0 ? 4 : 3);
                        const int by0 = dy < 0 ? -1 : (dy > 0 ? 4 : 0), by1 = dy < 0 ? -1 : (dy > 0 ? 4 : 3);
                        for (int by = by0; by <= by1; ++by) {
                            const int cy = ty * UT + by * 4 + 1;
                            if (cy < 0 || cy > sl.ny) continue;
                            for (int bx = bx0; bx <= bx1; ++bx) {
                                const int cx = tx * UT + bx * 4 + 1;
                                if (cx < 0 || cx > sl.nx) continue;
                                any = any || (s.bf_tile_charge[cell_index(sl, cx, cy)] == tg);
                            }
                        }
                    }
            }
            in_reach = any; bounds = any;
        }
    }
    const unsigned long long entry = pack_tile_entry(c, my_lo, my_t);
    {
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(in_reach);
        if (mask != 0ull) {
            int base = 0;
            if (lane == 0) base = atomicAdd(Ls.count + 2 * parity, (int)__popcll(mask));
            base = __shfl(base, 0, 64);
            if (in_reach) Ls.upd[base + (int)__popcll(mask & ((1ull << lane) - 1ull))] = entry;
        }
    }
    {
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(bounds);
        if (mask != 0ull) {
            int base = 0;
            if (lane == 0) base = atomicAdd(Ls.count + 2 * parity + 1, (int)__popcll(mask));
            base = __shfl(base, 0, 64);
            if (bounds) Ls.ref[base + (int)__popcll(mask & ((1ull << lane) - 1ull))] = entry;
        }
    }
}

// one listed tile
template <int NV>
__device__ __forceinline__ void update_listed_tile(const JointUpd* __restrict__ U, unsigned long long e, unsigned int tag, UpdateLds<NV>& L)
{
    int c, lo, t; unpack_tile_entry(e, c, lo, t);
    const ims_sensor_t& s = *U->sp[c];
    const ims_bf_slot_t bs = s.bf_slots[U->first_slot[c] + lo];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int tiles_x = tiles_across(sl.nx);
    const int tx0 = (t % tiles_x) * UT, ty0 = (t / tiles_x) * UT;
    const double* dl_global = U->dl[c];
#ifdef IMS_HIST
    const unsigned long long hist_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (dl_global != nullptr) update_tile_q3<NV, true, ConstTable>(s, sl, tx0, ty0, U->changed[c], L, false, tag, (ConstTable)(uintptr_t)dl_global);
    else update_tile_q3<NV, false>(s, sl, tx0, ty0, U->changed[c], L, false, tag);
#ifdef IMS_HIST
    __syncthreads();
    if (threadIdx.x == 0) {
        int halo = 0, own = 0;
        for (int hy = 0; hy < UpdateLds<NV>::HW; ++hy) {
            halo += __popc(L.occ[hy]);
            if (hy >= 4 && hy < 4 + UT) own += __popc((L.occ[hy] >> 4) & 0xFFFFu);
        }
        const int bin = halo < 63 ? halo : 63;
        atomicAdd(&g_hist[0][bin], 1ull);
        atomicAdd(&g_hist[1][bin], __builtin_amdgcn_s_memrealtime() - hist_t0);
        atomicAdd(&g_hist[2][bin], (unsigned long long)own);
    }
#endif
}

template <int NV, bool DPP = false>
__global__ __launch_bounds__(256, 5) void k_update_list_j(const JointUpd* __restrict__ U, const JointLists Ls, int parity, unsigned int tag,
                                                       int reset_next)
{
    __shared__ UpdateLds<NV> L0;
    const int n = Ls.count[2 * parity];
    // (search-side lists: no builder launch to empty the next round's list -- this launch sits between this round's search and the next's)
    if (reset_next && blockIdx.x == 0 && threadIdx.x == 0) { Ls.count[2 * (parity ^ 1)] = 0; Ls.count[2 * (parity ^ 1) + 1] = 0; }
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
        if (i != (int)blockIdx.x) __syncthreads();                  // the tile before is through with the shared buffers
        // (the address of the shared buffers through a register the compiler cannot look through: inside a loop it otherwise
        // keeps every one of the ~180 constant LDS addresses of the unrolled window in a register of its own -- 256 against 80)
        UpdateLds<NV>* Lp = &L0;
        asm volatile("" : "+v"(Lp));
        update_listed_tile<NV>(U, Ls.upd[i], tag, *Lp);
    }
}

template <int NV>
__global__ __launch_bounds__(256) void k_refresh_list_j(const JointUpd* __restrict__ U, const JointLists Ls, int parity, unsigned int tag,
                                                        int from_upd)
{
    // from_upd: ONE list for both (search-side lists: a tile is listed when charge lies within [t0 - 4, t0 + 19] of it, which covers
    // the update's halo and the right / upper neighbour's first column / row)
    const int n = Ls.count[2 * parity + (from_upd ? 0 : 1)];
    const unsigned long long* __restrict__ list = from_upd ? Ls.upd : Ls.ref;
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
        int c, lo, t; unpack_tile_entry(list[i], c, lo, t);
        const ims_sensor_t& s = *U->sp[c];
        const ims_bf_slot_t bs = s.bf_slots[U->first_slot[c] + lo];
        const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
        const int tiles_x = tiles_across(sl.nx);
        const int tx = t % tiles_x, ty = t / tiles_x;
        bool own, right, up, charged;
        if (!refresh_flags(s, { sl, tx, ty, tiles_x }, tag, own, right, up, charged)) continue;
        refresh_tile<NV>(s, sl, tx, ty, own, right, up, charged, (const unsigned char*)U->changed[c]);
    }
}

__global__ void k_clear_pristine(ims_sensor_t* sp) { sp->pristine_margin = -1.0; }

// ---------------- host side of the C-ABI ----------------
// ---- which photon kernel a launch gets: one selector, one table of instantiations ----
static bool has_optical_screen(const ims_render_params_t* p)
{
    for (int c = 0; c < p->n_psf; ++c)
        if (p->psf[c].kind == IMS_PSF_OPTICAL_SCREEN) return true;
    return false;
}
static bool psf_kinds_are(const ims_render_params_t* p, std::initializer_list<int32_t> kinds)
{
    int c = 0;
    for (const int32_t k : kinds)
        if (c >= p->n_psf || p->psf[c++].kind != k) return false;
    return c == p->n_psf;
}

// The template arguments of k_shoot_accumulate<CHAIN, PSF, LAYOUT> / k_shoot_photons<MODE, CHAIN, PSF, LAYOUT> for a descriptor.
// mode: 0 ims_shoot_photons, 1 ims_shoot_ops_photons on a pool that keeps directions and wavelengths, 2 the same on a converted
// pool and the fused kernel.  Reads n_ops, ops[].kind, n_psf, psf[].kind, atm, optics_layout and the tuning block, nothing else.
// CHAIN 1: the descriptor lists exactly imSim's default photon-op chain (run_ops<1>); only mode 2 has kernels for it.
// PSF 1: radial table then Gaussian (run_psf<1>); 2: phase screens, second-kick table, Gaussian (run_psf<2>: imSim's default
// AtmosphericPSF); 0: anything else.  (Variant 2 is slower than the component loop at four workgroups per CU -- C3b 36.9 -> 38.6 ms
// in round 2, 35.2 -> 35.9 ms now -- and faster at the three that launches with phase screens run with (photon_lds_pad):
// 33.7 -> 33.2 ms.  ims_tuning_t.psf_screens_kernel = 0 takes the loop.)
// 3: a list with an optical phase screen (IMS_PSF_OPTICAL_SCREEN) in it (run_psf<3>); 4: screens, second kick, optical screen,
// Gaussian -- AtmosphericPSF with doOpt (run_psf<4>), taken under the same switches as variant 2.  Lists without the component
// never reach a kernel compiled for it, and the other way round (a missing kernel is not replaced by another).
// The straight-line PSF forms 2 and 4 exist only with the unrolled ray trace of a known layout (ims_known_optics_layout): without
// it variant 2 runs the component loop on the default chain, variant 4 the loops over components, operators and surfaces.
// A perturbed telescope (include/imsim_hip.h) always takes the loops, every surface traced in its frame.
struct PhotonVariant { int chain; int psf; unsigned long long layout; };
static PhotonVariant select_photon_variant(const ims_render_params_t* p, int mode)
{
    static const int32_t chain[IMS_DEFAULT_CHAIN_LEN] = { IMS_OP_TIME_SAMPLER, IMS_OP_PUPIL_ANNULUS_SAMPLER, IMS_OP_PHOTON_DCR,
                                                          IMS_OP_RUBIN_DIFFRACTION_OPTICS, IMS_OP_FOCUS_DEPTH, IMS_OP_REFRACTION };
    const bool optical = has_optical_screen(p), pert = p->optics_layout == IMS_LAYOUT_PERTURBED;
    if (mode == 0) return { 0, optical ? 3 : 0, 0ull };
    if (mode == 1 || pert) return { 0, optical ? 3 : 0, pert ? IMS_LAYOUT_PERTURBED : 0ull };
    bool dc = p->n_ops == IMS_DEFAULT_CHAIN_LEN && g_tune.chain_kernels;
    for (int k = 0; dc && k < IMS_DEFAULT_CHAIN_LEN; ++k) dc = p->ops[k].kind == chain[k];
    const bool lay = dc && p->optics_layout == IMS_LAYOUT_RUBIN_LIKE && g_tune.layout_kernels != 0;
    const bool screens = g_tune.psf_screens_kernel != 0;
    if (optical) {
        if (lay && screens && psf_kinds_are(p, { IMS_PSF_SCREENS, IMS_PSF_RADIAL, IMS_PSF_OPTICAL_SCREEN, IMS_PSF_GAUSSIAN }))
            return { 1, 4, IMS_LAYOUT_RUBIN_LIKE };
        return { 0, 3, 0ull };
    }
    if (!dc) return { 0, 0, 0ull };
    if (psf_kinds_are(p, { IMS_PSF_RADIAL, IMS_PSF_GAUSSIAN })) return { 1, 1, lay ? IMS_LAYOUT_RUBIN_LIKE : 0ull };
    if (lay && screens && p->atm != nullptr && psf_kinds_are(p, { IMS_PSF_SCREENS, IMS_PSF_RADIAL, IMS_PSF_GAUSSIAN }))
        return { 1, 2, IMS_LAYOUT_RUBIN_LIKE };
    return { 1, 0, lay ? IMS_LAYOUT_RUBIN_LIKE : 0ull };
}

// Every (CHAIN, PSF, LAYOUT) the library holds photon kernels for.  ims_shoot_photons (MODE 0) has the two loop forms without a
// layout, a pool that is not converted (MODE 1) those and their perturbed forms, the fused kernel and MODE 2 all ten.
#define IMS_PHOTON_VARIANTS_MODE0(X) X(0, 0, 0ull) X(0, 3, 0ull)
#define IMS_PHOTON_VARIANTS_MODE1(X) IMS_PHOTON_VARIANTS_MODE0(X) X(0, 0, IMS_LAYOUT_PERTURBED) X(0, 3, IMS_LAYOUT_PERTURBED)
#define IMS_PHOTON_VARIANTS_MODE2(X) IMS_PHOTON_VARIANTS_MODE1(X) X(1, 0, 0ull) X(1, 1, 0ull) X(1, 0, IMS_LAYOUT_RUBIN_LIKE) \
    X(1, 1, IMS_LAYOUT_RUBIN_LIKE) X(1, 2, IMS_LAYOUT_RUBIN_LIKE) X(1, 4, IMS_LAYOUT_RUBIN_LIKE)

template <int CHAIN, int PSF, unsigned long long LAYOUT>
struct PhotonKernel { static constexpr int chain = CHAIN, psf = PSF; static constexpr unsigned long long layout = LAYOUT; };

// launch(PhotonKernel<CHAIN, PSF, LAYOUT>{}) for the row of the mode's list that is v: a triple the list does not hold is an
// error, never another kernel
template <int MODE, class Launch>
static int launch_photon_variant(const PhotonVariant& v, Launch&& launch)
{
#define IMS_TRY_VARIANT(C, F, L) if (v.chain == C && v.psf == F && v.layout == L) { launch(PhotonKernel<C, F, L>{}); return IMS_OK; }
    if constexpr (MODE == 0) { IMS_PHOTON_VARIANTS_MODE0(IMS_TRY_VARIANT) }
    else if constexpr (MODE == 1) { IMS_PHOTON_VARIANTS_MODE1(IMS_TRY_VARIANT) }
    else { IMS_PHOTON_VARIANTS_MODE2(IMS_TRY_VARIANT) }
#undef IMS_TRY_VARIANT
    char msg[160];
    snprintf(msg, sizeof(msg), "no photon kernel <CHAIN %d, PSF %d, LAYOUT 0x%llx> for mode %d", v.chain, v.psf, v.layout, MODE);
    return set_err(IMS_ERR_UNSUPPORTED, msg);
}
// what ims_accumulate_segments / _small / _round ask of the pool and the image they deposit it into
static int check_pooled_accumulate(const ims_render_params_t* params, const ims_photons_t* pool, const int64_t* pool_start)
{
    if (!pool || !pool_start) return set_err(IMS_ERR_ARG, "pool/pool_start is NULL");
    if (!pool->converted) return set_err(IMS_ERR_ARG, "pool must hold converted photons (ims_shoot_ops_photons with pool->converted = 1)");
    if (!params->image) return set_err(IMS_ERR_ARG, "image is NULL");
    if (params->lazy_static) return set_err(IMS_ERR_ARG, "lazy_static parameters (slot 0 holds no state) belong to ims_shoot_accumulate only");
    return IMS_OK;
}

extern "C" {

int ims_photon_kernel_variant(const ims_render_params_t* params, int32_t mode, int32_t* chain, int32_t* psf, uint64_t* layout)
{
    if (!params || !chain || !psf || !layout) return set_err(IMS_ERR_ARG, "params / chain / psf / layout is NULL");
    if (mode < 0 || mode > 2) return set_err(IMS_ERR_ARG, "mode must be 0, 1 or 2");
    const PhotonVariant v = select_photon_variant(params, mode);
    *chain = v.chain; *psf = v.psf; *layout = v.layout;
    return IMS_OK;
}

int ims_known_optics_layout(uint64_t layout) { return layout == IMS_LAYOUT_RUBIN_LIKE ? 1 : 0; }

// Dynamic LDS a photon-kernel launch asks for without using it: with more than a quarter of a CU's 160 KB per workgroup only
// three photon workgroups are resident per CU.  Launches whose PSF gathers phase screens are bound by those scattered loads, not
// by instruction issue, and run 2.5 % faster that way (C3b 34.7 -> 33.8 ms: fewer wavefronts thrash the caches less); the
// analytic-PSF kernels are issue-bound and lose 9 % (C4 237 -> 258 ms; the free fourth slot does not buy the brighter-fatter
// chains enough: C3 23.6 -> 25.4 ms), so they ask for none.  ims_tuning_t.photon_lds >= 0 (bytes) overrides both.
static unsigned photon_lds_pad(const ims_render_params_t* p)
{
    if (g_tune.photon_lds >= 0 && g_tune.photon_lds <= 65536 - 4096) return (unsigned)g_tune.photon_lds;
    for (int c = 0; c < p->n_psf; ++c)
        if (p->psf[c].kind == IMS_PSF_SCREENS && p->atm != nullptr && p->screen_kick == nullptr) return 41984u;
    return 0u;
}

int ims_shoot_accumulate(const ims_render_params_t* params_in, void* stream)
{
    int rc = check_params(params_in);
    if (rc) return rc;
    if (!params_in->image) return set_err(IMS_ERR_ARG, "image is NULL");
    if (params_in->n_segments == 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    ims_render_params_t lazy_copy;
    const ims_render_params_t* params = params_in;
    if (params_in->lazy_static) {
        if (!params_in->sensor || params_in->track_static_delta)
            return set_err(IMS_ERR_ARG, "lazy_static needs a Silicon sensor whose slot 0 is not a live region (track_static_delta 0)");
        const int64_t want = params_in->n_segments * (int64_t)params_in->seg_size;
        if (want > (int64_t)1 << 26) return set_err(IMS_ERR_UNSUPPORTED, "lazy_static: more than 2^26 photons in one launch");
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        MarginBuf mb;
        {
            std::lock_guard<std::mutex> lock(g_state_mutex);
            MarginBuf& m = g_margin[std::make_pair(dev, stream)];
            const int64_t waves = params_in->n_segments * 4;
            if (m.cap < (uint32_t)want || m.waves_cap < waves) {
                // grown into temporaries and committed only when every allocation has succeeded: an entry left with freed
                // pointers and the new capacities would pass this very check on the next call
                if (!m.count) HIP_TRY(hipMalloc((void**)&m.count, 2 * sizeof(int32_t)));
                const uint32_t cap = (uint32_t)(want + want / 4 + 65536);
                const int64_t waves_cap = waves + waves / 4 + 1024;
                double* list = nullptr;
                unsigned char* wave_count = nullptr;
                // an octet of records per wavefront, then an overflow region that could take every photon of the launch
                HIP_TRY(hipMalloc((void**)&list, ((size_t)waves_cap * 8 + (size_t)cap) * 5 * sizeof(double)));
                const hipError_t e2 = hipMalloc((void**)&wave_count, (size_t)waves_cap);
                if (e2 != hipSuccess) { (void)hipFree(list); return hip_err(e2, "hipMalloc(margin wave counts)"); }
                if (m.list) { (void)hipFree(m.list); (void)hipFree(m.wave_count); }
                m.list = list; m.wave_count = wave_count; m.cap = cap; m.waves_cap = waves_cap;
            }
            mb = m;
        }
        lazy_copy = *params_in;
        lazy_copy.margin_list = mb.list; lazy_copy.margin_count = mb.count; lazy_copy.margin_cap = mb.cap;
        lazy_copy.margin_wave_count = mb.wave_count; lazy_copy.margin_waves = params_in->n_segments * 4;
        params = &lazy_copy;
        HIP_TRY(hipMemsetAsync(mb.count, 0, 2 * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(mb.wave_count, 0, (size_t)lazy_copy.margin_waves, st));
    }
    {
        LaunchTimer tm(st, 1);
        const dim3 grid(grid_for_segments(params->n_segments));
        rc = launch_photon_variant<2>(select_photon_variant(params, 2), [&](auto k) {
            using K = decltype(k);
            hipLaunchKernelGGL((k_shoot_accumulate<K::chain, K::psf, K::layout>), grid, dim3(256), photon_lds_pad(params), st, *params);
        });
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    if (params->lazy_static) {
        // the photons set aside (~2 % of the launch's): one lane each, the polygons evaluated on the way
        hipLaunchKernelGGL(k_margin_photons, dim3(1024), dim3(256), 0, st, *params);
        HIP_TRY(hipGetLastError());
    }
    return IMS_OK;
}

int ims_shoot_photons(const ims_render_params_t* params, const int64_t* photon_offset,
                      const ims_photons_t* pool, void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (!photon_offset || !pool) return set_err(IMS_ERR_ARG, "photon_offset/pool is NULL");
    if (params->n_segments == 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    rc = launch_photon_variant<0>(select_photon_variant(params, 0), [&](auto k) {
        using K = decltype(k);
        hipLaunchKernelGGL((k_shoot_photons<0, K::chain, K::psf, K::layout>), dim3(grid_for_segments(params->n_segments)), dim3(256), 0, st,
                           *params, photon_offset, *pool);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_shoot_ops_photons(const ims_render_params_t* params, const int64_t* photon_offset,
                          const ims_photons_t* pool, void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (!photon_offset || !pool) return set_err(IMS_ERR_ARG, "photon_offset/pool is NULL");
    if (!pool->x || !pool->y || !pool->flux || !pool->dxdz) return set_err(IMS_ERR_ARG, "pool: x / y / flux / dxdz is NULL");
    if (!pool->converted && (!pool->dydz || !pool->wavelength)) return set_err(IMS_ERR_ARG, "pool: dydz / wavelength is NULL");
    if (params->n_segments == 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    {
        LaunchTimer tm(st, 2);
        const dim3 grid(grid_for_segments(params->n_segments));
        const unsigned lds = photon_lds_pad(params);
        if (pool->converted)
            rc = launch_photon_variant<2>(select_photon_variant(params, 2), [&](auto k) {
                using K = decltype(k);
                hipLaunchKernelGGL((k_shoot_photons<2, K::chain, K::psf, K::layout>), grid, dim3(256), lds, st, *params, photon_offset, *pool);
            });
        else
            rc = launch_photon_variant<1>(select_photon_variant(params, 1), [&](auto k) {
                using K = decltype(k);
                hipLaunchKernelGGL((k_shoot_photons<1, K::chain, K::psf, K::layout>), grid, dim3(256), lds, st, *params, photon_offset, *pool);
            });
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_psf_moments(const ims_render_params_t* params, int32_t stage, double* partial_dev, double* sums_dev, int64_t* counts_dev,
                    void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (stage != 1 && stage != 2) return set_err(IMS_ERR_ARG, "psf_moments: stage must be 1 (shoot + PSF) or 2 (+ photon operators)");
    if (params->n_objects == 0) return IMS_OK;
    if (!sums_dev || !counts_dev) return set_err(IMS_ERR_ARG, "psf_moments: sums / counts is NULL");
    if (params->n_segments > 0 && !partial_dev) return set_err(IMS_ERR_ARG, "psf_moments: partial is NULL");
    if (params->n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_moments: too many points for one call");
    hipStream_t st = (hipStream_t)stream;
    if (params->n_segments > 0) {
        // the kernels of a pool that is not converted (mode 1): the loops over the descriptors, whose photons these are
        const dim3 grid(grid_for_segments(params->n_segments));
        const unsigned lds = photon_lds_pad(params);
        rc = launch_photon_variant<1>(select_photon_variant(params, 1), [&](auto k) {
            using K = decltype(k);
            hipLaunchKernelGGL((k_psf_moments<K::chain, K::psf, K::layout>), grid, dim3(256), lds, st, *params, (int)stage, partial_dev);
        });
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_psf_moments_combine, dim3((unsigned)params->n_objects), dim3(256), 0, st, params->seg_prefix, partial_dev,
                       sums_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_accumulate_segments(const ims_render_params_t* params, const ims_photons_t* pool, const int64_t* pool_start,
                            int32_t num_vertices, void* stream)
{
    int rc = check_params(params);
    if (!rc) rc = check_pooled_accumulate(params, pool, pool_start);
    if (rc) return rc;
    if (params->n_segments == 0) return IMS_OK;
    const dim3 grid(grid_for_segments(params->n_segments));
    with_nv(num_vertices, [&](auto nv) {
        hipLaunchKernelGGL(k_accumulate_segments<decltype(nv)::value>, grid, dim3(256), 0, (hipStream_t)stream, *params, *pool, pool_start);
    });
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_accumulate_small(const ims_render_params_t* params, const ims_photons_t* pool, const int64_t* pool_start,
                         int32_t num_vertices, void* stream)
{
    if (!params) return set_err(IMS_ERR_ARG, "params is NULL");
    if (!params->objects || !params->image) return set_err(IMS_ERR_ARG, "objects/image is NULL");
    const int rc = check_pooled_accumulate(params, pool, pool_start);
    if (rc) return rc;
    if (params->n_objects <= 0) return IMS_OK;
    const int64_t blocks = (params->n_objects + 3) / 4;
    if (blocks > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "too many objects for one launch");
    const dim3 grid((unsigned)blocks);
    with_nv(num_vertices, [&](auto nv) {
        hipLaunchKernelGGL(k_accumulate_small<decltype(nv)::value>, grid, dim3(256), 0, (hipStream_t)stream, *params, *pool, pool_start);
    });
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_accumulate_round(const ims_render_params_t* params, const ims_photons_t* pool, const int64_t* pool_start,
                         int32_t round, int32_t nrecalc, int32_t n_active, int32_t num_vertices, void* stream)
{
    if (!params) return set_err(IMS_ERR_ARG, "params is NULL");
    if (!params->objects || !params->image) return set_err(IMS_ERR_ARG, "objects/image is NULL");
    const int rc = check_pooled_accumulate(params, pool, pool_start);
    if (rc) return rc;
    if (round < 0 || nrecalc <= 0) return set_err(IMS_ERR_ARG, "round must be >= 0 and nrecalc positive");
    if (n_active < 0 || n_active > params->n_objects) return set_err(IMS_ERR_ARG, "n_active out of range");
    if (n_active == 0) return IMS_OK;
    // (One-wavefront workgroups for this launch -- a 256-thread workgroup starts only where a compute unit has a free register slot on
    // each of its four SIMDs at once, and the pixel search of a round waited ~220 us for that beside the photon kernels -- were built
    // and measured in round 4: the wait disappears and the photon kernels lose what the chain gains, C3 24.0 -> 25.8 ms; removed.)
    const int32_t segs = (nrecalc + 255) / 256;
    if ((int64_t)n_active * segs > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "too many workgroups for one round");
    const dim3 grid((unsigned)(n_active * segs));
    const int64_t first = (int64_t)round * nrecalc;
    LaunchTimer tm((hipStream_t)stream, 4);
    with_nv(num_vertices, [&](auto nv) {
        hipLaunchKernelGGL(k_accumulate_round<decltype(nv)::value>, grid, dim3(256), 0, (hipStream_t)stream, *params, *pool, pool_start, first,
                           nrecalc, segs);
    });
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

static RoundArgs round_args(const ims_render_params_t& P, const ims_photons_t& pool)
{
    return { P.objects, P.sensor, P.image, P.realized_flux, pool.x, pool.y, pool.flux, pool.dxdz, P.nx, P.ny, P.xmin, P.ymin,
             P.bf_tag, P.bf_slot_shift, P.track_static_delta, 0 };
}

// ims_accumulate_round launched with the compact argument block (4 vertices per edge, 256-thread workgroups)
static int accumulate_round_compact(const ims_render_params_t* params, const ims_photons_t* pool, const int64_t* pool_start, int32_t round,
                                    int32_t nrecalc, int32_t n_active, int32_t num_vertices, void* stream)
{
    if (n_active == 0) return IMS_OK;
    if (num_vertices != 4 || !g_tune.round_compact)
        return ims_accumulate_round(params, pool, pool_start, round, nrecalc, n_active, num_vertices, stream);
    if (!params || !params->objects || !params->image || !pool || !pool_start || !pool->converted) return set_err(IMS_ERR_ARG, "NULL argument");
    const int32_t segs = (nrecalc + 255) / 256;
    if ((int64_t)n_active * segs > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "too many workgroups for one round");
    const RoundArgs a = round_args(*params, *pool);
    LaunchTimer tm((hipStream_t)stream, 4);
    if (g_tune.round_two_segments) {
        const int32_t segs2 = (nrecalc + 511) / 512;
        hipLaunchKernelGGL((k_accumulate_round_c2<4>), dim3((unsigned)(n_active * segs2)), dim3(256), 0, (hipStream_t)stream, a, pool_start,
                           (int64_t)round * nrecalc, nrecalc, segs2);
    } else
    hipLaunchKernelGGL((k_accumulate_round_c<4, 256>), dim3((unsigned)(n_active * segs)), dim3(256), 0, (hipStream_t)stream, a, pool_start,
                       (int64_t)round * nrecalc, nrecalc, segs);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_apply_ops(const ims_render_params_t* params, const int64_t* photon_offset, const ims_photons_t* pool, void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (!photon_offset || !pool) return set_err(IMS_ERR_ARG, "photon_offset/pool is NULL");
    if (pool->n == 0 || params->n_ops == 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    {
        if (params->optics_layout == IMS_LAYOUT_PERTURBED)
            hipLaunchKernelGGL((k_apply_ops<IMS_LAYOUT_PERTURBED>), dim3(grid_for_pool(pool->n)), dim3(256), 0, st, *params, photon_offset, *pool);
        else
            hipLaunchKernelGGL((k_apply_ops<0>), dim3(grid_for_pool(pool->n)), dim3(256), 0, st, *params, photon_offset, *pool);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_accumulate(const ims_render_params_t* params, const int64_t* photon_offset, const ims_photons_t* pool,
                   int32_t* pixel_index_out, void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (!photon_offset || !pool) return set_err(IMS_ERR_ARG, "photon_offset/pool is NULL");
    if (!params->image) return set_err(IMS_ERR_ARG, "image is NULL");
    if (params->lazy_static) return set_err(IMS_ERR_ARG, "lazy_static parameters (slot 0 holds no state) belong to ims_shoot_accumulate only");
    if (pool->n == 0) return IMS_OK;
    hipStream_t st = (hipStream_t)stream;
    {
        hipLaunchKernelGGL(k_accumulate, dim3(grid_for_pool(pool->n)), dim3(256), 0, st, *params, photon_offset, *pool,
                           pixel_index_out);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

static int slot_range_cells(const ims_sensor_t* host, int first, int n, int64_t* begin, int64_t* count)
{
    if (!host || !host->bf_slots) return set_err(IMS_ERR_ARG, "sensor_host/bf_slots is NULL (host copy of the slot table required)");
    if (n <= 0 || first < 0 || first + n > host->n_bf_slots) return set_err(IMS_ERR_ARG, "slot range out of bounds");
    const ims_bf_slot_t& a = host->bf_slots[first];
    const ims_bf_slot_t& z = host->bf_slots[first + n - 1];
    *begin = a.offset;
    *count = z.offset + (int64_t)(z.nx + 1) * (z.ny + 1) - a.offset;
    return IMS_OK;
}

int ims_sensor_init_boundaries(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host,
                               int32_t first_slot, int32_t n_slots, const int64_t* tile_prefix_dev, int64_t n_tiles, void* stream)
{
    if (!sensor_dev) return set_err(IMS_ERR_ARG, "sensor_dev is NULL");
    if (n_slots == 0) return IMS_OK;
    int64_t begin, count;
    int rc = slot_range_cells(sensor_host, first_slot, n_slots, &begin, &count);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (sensor_host->num_vertices == IT_NV && g_tune.init_tiles && tile_prefix_dev != nullptr) {
        if (n_tiles <= 0 || n_tiles > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "n_tiles out of range");
        hipLaunchKernelGGL(k_init_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, sensor_dev, first_slot, n_slots, tile_prefix_dev);
        HIP_TRY(hipGetLastError());
        return IMS_OK;
    }
    if (sensor_host->num_vertices == IT_NV && g_tune.init_tiles) {
        // tiled kernel: grid.x = the largest tile count of a run of consecutive slots, grid.y = the slots of the run (at most
        // 65 535); a run ends where the workgroups that find no tile would outnumber the working ones four to one
        int a = first_slot;
        const int end = first_slot + n_slots;
        while (a < end) {
            auto tiles_of = [&](int k) {
                const ims_bf_slot_t& b = sensor_host->bf_slots[k];
                return (int64_t)tiles_across(b.nx) * tiles_across(b.ny);
            };
            int64_t hi = tiles_of(a), sum = hi;
            int z = a + 1;
            while (z < end && z - a < 65535) {
                const int64_t tz = tiles_of(z);
                const int64_t nhi = tz > hi ? tz : hi;
                if (nhi * (z - a + 1) > 4 * (sum + tz) + 4096) break;
                hi = nhi; sum += tz; ++z;
            }
            if (hi > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "slot too large");
            hipLaunchKernelGGL(k_init_tiles, dim3((unsigned)hi, (unsigned)(z - a)), dim3(256), 0, st, sensor_dev, a, z - a,
                               (const int64_t*)nullptr);
            a = z;
        }
        HIP_TRY(hipGetLastError());
        return IMS_OK;
    }
    const unsigned g = (unsigned)((count + 255) / 256);
    hipLaunchKernelGGL(k_init_boundaries, dim3(g), dim3(256), 0, st, sensor_dev, first_slot, n_slots, begin, count);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

static int update_distortions_impl(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host,
                                   int32_t first_slot, int32_t n_slots, const int64_t* tile_prefix_dev,
                                   int64_t n_tiles, unsigned char* changed_dev, uint32_t tag, double* fold_image, void* stream)
{
    if (!sensor_dev) return set_err(IMS_ERR_ARG, "sensor_dev is NULL");
    if (n_slots == 0) return IMS_OK;
    if (!tile_prefix_dev || !changed_dev) return set_err(IMS_ERR_ARG, "tile_prefix/changed is NULL");
    if (sensor_host && sensor_host->qdist > UQMAX) return set_err(IMS_ERR_UNSUPPORTED, "qdist > 4 not supported");
    if (sensor_host && (sensor_host->qdist < 0 || 2 * sensor_host->qdist + 1 > sensor_host->nx || 2 * sensor_host->qdist + 1 > sensor_host->ny))
        return set_err(IMS_ERR_UNSUPPORTED, "qdist reaches beyond the tabulated stamp of the sensor model");
    int64_t begin, count;
    int rc = slot_range_cells(sensor_host, first_slot, n_slots, &begin, &count);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (first_slot == 0)                      // slot 0 leaves its pristine state: photons must consult the boundaries again
        hipLaunchKernelGGL(k_clear_pristine, dim3(1), dim3(1), 0, st, const_cast<ims_sensor_t*>(sensor_dev));
    const unsigned g = (unsigned)((count + 255) / 256);
    const int nV = sensor_host ? sensor_host->num_vertices : 0;
    const int q = sensor_host ? sensor_host->qdist : 0;
    // The DPP form of the update is the faster one where a round's latency counts (a few tiles: 14.2 -> 11.0 us per launch for
    // one star), the SGPR form where a launch is throughput work beside the photon kernels (its waves sleep on the scalar
    // cache instead of pulling 10 KB of table through LDS per tile: C3 25.0 against 25.9 ms): the tile count decides.
    const bool dpp = sensor_host && sensor_host->bf_dl != nullptr && g_tune.upd_dpp && n_tiles <= g_tune.upd_dpp_max;
    const dim3 grid((unsigned)n_tiles);
    with_nv(nV, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if constexpr (NV != 0) {                                                      // (the q3 update has no form for other counts)
            if (q == 3) {
                hipLaunchKernelGGL((dpp ? k_update_distortions_q3<NV, true> : k_update_distortions_q3<NV, false>), grid, dim3(256), 0, st,
                                   sensor_dev, first_slot, n_slots, tile_prefix_dev, changed_dev, tag, sensor_host->bf_dl);
                return;
            }
        }
        hipLaunchKernelGGL(k_update_distortions, grid, dim3(256), 0, st, sensor_dev, first_slot, n_slots, tile_prefix_dev, changed_dev, tag);
    });
    with_nv(nV, [&](auto nv) {
        hipLaunchKernelGGL(k_refresh_changed<decltype(nv)::value>, grid, dim3(256), 0, st, sensor_dev, first_slot, n_slots, tile_prefix_dev,
                           (const unsigned char*)changed_dev, tag, fold_image);
    });
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_sensor_update_distortions(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host,
                                  int32_t first_slot, int32_t n_slots, const int64_t* tile_prefix_dev,
                                  int64_t n_tiles, unsigned char* changed_dev, uint32_t tag, void* stream)
{
    return update_distortions_impl(sensor_dev, sensor_host, first_slot, n_slots, tile_prefix_dev, n_tiles, changed_dev, tag, nullptr, stream);
}

// slot `slot` must be the pixel grid of the image (nx x ny): what the fold forms index with
static int fold_geometry(const ims_sensor_t* sensor_host, int32_t slot, double* image_dev, int32_t nx, int32_t ny)
{
    if (!image_dev) return set_err(IMS_ERR_ARG, "image is NULL");
    if (!sensor_host || !sensor_host->bf_slots || slot < 0 || slot >= sensor_host->n_bf_slots)
        return set_err(IMS_ERR_ARG, "sensor_host / its slot table is NULL or the slot is out of range");
    const ims_bf_slot_t& b = sensor_host->bf_slots[slot];
    if (b.nx != nx || b.ny != ny) return set_err(IMS_ERR_ARG, "the slot is not the pixel grid of the image (nx / ny differ)");
    return IMS_OK;
}

int ims_sensor_update_distortions_fold(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host, const int64_t* tile_prefix_dev,
                                       int64_t n_tiles, unsigned char* changed_dev, uint32_t tag, double* image_dev, int32_t nx, int32_t ny,
                                       void* stream)
{
    const int rc = fold_geometry(sensor_host, 0, image_dev, nx, ny);
    if (rc) return rc;
    return update_distortions_impl(sensor_dev, sensor_host, 0, 1, tile_prefix_dev, n_tiles, changed_dev, tag, image_dev, stream);
}

__global__ __launch_bounds__(256) void k_fold_delta(const ims_sensor_t* __restrict__ sp, int slot, double* __restrict__ image)
{
    const ims_sensor_t& s = *sp;
    const ims_bf_slot_t bs = s.bf_slots[slot];
    const int64_t n = (int64_t)bs.nx * bs.ny, stride = (int64_t)gridDim.x * 256;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += stride) {
        const int i = (int)(p % bs.nx), j = (int)(p / bs.nx);
        const int64_t c = bs.offset + (int64_t)j * (bs.nx + 1) + i;
        const double d = s.bf_delta[c];
        if (d != 0.0) { image[p] += d; s.bf_delta[c] = 0.0; }
    }
}

int ims_sensor_fold_delta(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host, int32_t slot, double* image_dev, int32_t nx,
                          int32_t ny, void* stream)
{
    if (!sensor_dev) return set_err(IMS_ERR_ARG, "sensor_dev is NULL");
    const int rc = fold_geometry(sensor_host, slot, image_dev, nx, ny);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fold_delta, dim3(4096), dim3(256), 0, (hipStream_t)stream, sensor_dev, slot, image_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"

#include "ims_image.h"          // LSST_Flat and image utilities: pixel areas, flats, image add / convert, cosmic rays
#include "ims_fft_branch.h"     // the FFT branch: k-space fill, hipFFT plan cache and inverse, diffraction spikes, finish
#include "ims_table.h"          // the object table on the device: build, patch stamp sizes, gather rows
#include "ims_plan_run.h"       // plan items, the LSST_Image launch planner (ims_plan.h) bound and run, joint runs of a visit
#include "ims_opd.h"            // wavefront maps, annular-Zernike normal equations and field-point traces
#include "ims_sed.h"            // per-object SEDs through the bandpass
#include "ims_readout.h"        // CCD readout: bleed trails, amplifier segments, CTE, noise and digitisation
#include "ims_screen.h"         // phase-screen pre-pass
#include "ims_derive.h"         // derived constants of the descriptors (host only)
#include "ims_instcat.h"        // instance-catalog tokenizer (host only)
#include "ims_knots.h"          // RandomKnots on the FFT branch: knot positions and the structure-factor pass
#include "ims_stamp_fft.h"      // FITS stamps on the FFT branch: the pixel spectrum times the interpolant's transform
#include "ims_profile.h"        // radial / azimuthal histograms of the delivered PSF (the photons of ims_psf_moments, binned)
#include "ims_psf_image.h"      // postage stamps of the same photons, binned up to the sensor's conversion and diffusion
#include "ims_adaptive.h"       // adaptive (elliptical-Gaussian-weighted) moments of the same photons, iterated on the device
#include "ims_reshoot.h"        // FFT-drawn stamps re-shot through the photon operators (stamp.fft_photon_ops behind stamp.fft_reshoot)
#include "ims_exchange.h"       // RCCL exchanges between the GPUs of a node
#include "ims_test.h"           // device probes of the parity tests
