// mc_gs.hip -- multicolour Gauss-Seidel: the colour-major sliced format of a
// coloured operator, built on the device, and its two sweeps -- a launch per colour (any number
// of ranks) and one workgroup that keeps x in LDS (levels without a halo exchange).
//
// One sweep visits the colours in order; a row i of the colour takes
//   x_i = x_i + dinv_i * (b_i - s),  s = 0, s += a_ik * x_k in CSR order (no FMA: the file is
// compiled with -ffp-contract=off), dinv_i = 1.0 / a_ii
// reading the current x.  Rows of one colour never read each other, so every form below gives
// the bits of the definition.
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstdlib>

#include "device.hpp"

namespace amg {

namespace {

struct McArgs {
    const int4* slices;  // {first position in rows, rows, offset / 64, width}
    const int* rows;     // colour-major row list
    const int* col;      // -1 = padding
    const double* val;
    const double* dinv;  // by position in rows
    const double* b;
    double* x;           // in place
    const double* xh;    // halo values (columns >= ncl)
    int ncl;
};

// x as a sweep reads it: the vector and its halo in global memory, or the workgroup's LDS copy
struct XGlobal {
    const double* x;
    const double* xh;
    int ncl;
    __device__ __forceinline__ double operator()(int c) const { return c < ncl ? x[c] : xh[c - ncl]; }
};
struct XLds {
    const double* x;
    __device__ __forceinline__ double operator()(int c) const { return x[c]; }
};

__device__ __forceinline__ double mc_bcast(double v, int lane) {
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)bits, lane);
    const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// a lane colour's slice: lane = row, its entries a coalesced column-major stream, 8 in flight
template <class X>
__device__ __forceinline__ void mc_lane_slice(const McArgs& a, const int4 sl, int lane, const X& xr, double* xw) {
    constexpr int U = 8;
    const size_t base = (size_t)sl.z * 64 + lane;
    const int* colp = a.col + base;
    const double* valp = a.val + base;
    double s = 0.0;
    for (int k0 = 0; k0 < sl.w; k0 += U) {
        int c[U];
        double v[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = k0 + u < sl.w;  // uniform
            c[u] = in ? __builtin_nontemporal_load(colp + (size_t)(k0 + u) * 64) : -1;
            v[u] = in ? __builtin_nontemporal_load(valp + (size_t)(k0 + u) * 64) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = c[u] >= 0 ? xr(c[u]) : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0) s += v[u] * xv[u];  // padding is masked, never multiplied
    }
    if (lane < sl.y) {
        const int r = a.rows[sl.x + lane];
        xw[r] = xw[r] + a.dinv[sl.x + lane] * (a.b[r] - s);
    }
}

// a wave colour's slice: one row, 64 products at a time, added by every lane in CSR order
template <class X>
__device__ __forceinline__ void mc_wave_slice(const McArgs& a, const int4 sl, int lane, const X& xr, double* xw) {
    const size_t base = (size_t)sl.z * 64 + lane;
    double s = 0.0;
    for (int k0 = 0; k0 < sl.w; k0 += 64) {
        const int c = a.col[base + k0];  // the row is padded to whole 64s
        const double p = c >= 0 ? a.val[base + k0] * xr(c) : 0.0;
        const int m = min(64, sl.w - k0);  // uniform: the entries of this round
        for (int t = 0; t < m; ++t) s += mc_bcast(p, t);
    }
    if (lane == 0) {
        const int r = a.rows[sl.x];
        xw[r] = xw[r] + a.dinv[sl.x] * (a.b[r] - s);
    }
}

// slices [s0, s1) of one colour, a wave per slice
template <bool WAVE>
__global__ __launch_bounds__(kTPB) void mc_gs_colour_kernel(McArgs a, int s0, int s1) {
    const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6))) + s0;
    if (q >= s1) return;
    const int lane = threadIdx.x & 63;
    const int4 sl = a.slices[q];
    const XGlobal xr{a.x, a.xh, a.ncl};
    if (WAVE) mc_wave_slice(a, sl, lane, xr, a.x);
    else mc_lane_slice(a, sl, lane, xr, a.x);
}

// The whole sweep in one workgroup (no halo, n <= kMcWgCapacity rows): x lives in LDS, the
// waves share a colour's slices, a barrier separates the colours.  The arithmetic of every row
// is mc_gs_colour_kernel's
__global__ __launch_bounds__(kMcWgThreads) void mc_gs_wg_kernel(McArgs a, const int* cslice, const uint8_t* wave,
                                                                int nc, int n, int backward) {
    extern __shared__ double mc_xs[];
    for (int i = threadIdx.x; i < n; i += kMcWgThreads) mc_xs[i] = a.x[i];
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const XLds xr{mc_xs};
    for (int t = 0; t < nc; ++t) {
        const int c = backward ? nc - 1 - t : t;
        const int s0 = cslice[c], s1 = cslice[c + 1];
        const bool wv = wave[c] != 0;
        for (int q = s0 + w; q < s1; q += kMcWgThreads / 64) {
            const int4 sl = a.slices[q];
            if (wv) mc_wave_slice(a, sl, lane, xr, mc_xs);
            else mc_lane_slice(a, sl, lane, xr, mc_xs);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += kMcWgThreads) a.x[i] = mc_xs[i];
}

// ---- the format, built on the device -------------------------------------------------------
__global__ void mc_iota_kernel(int n, int* out) {
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i < n) out[i] = i;
}

// per slice: its width (longest row) and its cells in units of 64
__global__ void mc_width_kernel(int ns, const int2* span, const uint8_t* swave, const int* rows, const int* rp,
                                int* width, int* cells) {
    const int q = blockIdx.x * kTPB + threadIdx.x;
    if (q >= ns) return;
    int w = 0;
    for (int t = 0; t < span[q].y; ++t) {
        const int r = rows[span[q].x + t];
        w = max(w, rp[r + 1] - rp[r]);
    }
    width[q] = w;
    cells[q] = swave[q] ? (w + 63) / 64 : w;
}

// a wave per slice: the slice header, its rows' entries in CSR order, -1 in every other cell,
// and 1 / a_ii by position
__global__ __launch_bounds__(kTPB) void mc_fill_kernel(int ns, const int2* span, const uint8_t* swave, const int* rows,
                                                       const int* rp, const int* ccol, const double* cval,
                                                       const double* dinv_row, const int* width, const int* off,
                                                       int4* slices, int* col, double* val, double* dinv) {
    const int q = blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6);
    if (q >= ns) return;
    const int lane = threadIdx.x & 63;
    const int2 sp = span[q];
    const int w = width[q];
    const size_t base = (size_t)off[q] * 64;
    if (lane == 0) slices[q] = make_int4(sp.x, sp.y, off[q], w);
    if (swave[q]) {
        const int r = rows[sp.x];
        const int k0 = rp[r];
        for (int k = lane; k < (w + 63) / 64 * 64; k += 64) {
            col[base + k] = k < w ? ccol[k0 + k] : -1;
            val[base + k] = k < w ? cval[k0 + k] : 0.0;
        }
        if (lane == 0) dinv[sp.x] = dinv_row[r];
        return;
    }
    const bool live = lane < sp.y;
    const int r = live ? rows[sp.x + lane] : 0;
    const int k0 = live ? rp[r] : 0, len = live ? rp[r + 1] - k0 : 0;
    for (int k = 0; k < w; ++k) {
        col[base + (size_t)k * 64 + lane] = k < len ? ccol[k0 + k] : -1;
        val[base + (size_t)k * 64 + lane] = k < len ? cval[k0 + k] : 0.0;
    }
    if (live) dinv[sp.x + lane] = dinv_row[r];
}

inline unsigned grid_of(long long n, int per) { return (unsigned)std::max<long long>(1, (n + per - 1) / per); }

}  // namespace

// rows up to which the automatic path sweeps in one workgroup: kMcWgRows, or AMG_MC_GS_WG_ROWS
// from the environment (0: never; clipped to the LDS capacity) -- the knob the threshold was
// measured with (profiles/mc_gs)
int mc_wg_rows() {
    static const int v = [] {
        const char* e = std::getenv("AMG_MC_GS_WG_ROWS");
        return e && *e ? std::min(std::max(std::atoi(e), 0), kMcWgCapacity) : kMcWgRows;
    }();
    return v;
}

bool DevMatrix::mc_one_wg_fits() const {
    return (ctx->host.nranks == 1 || replicated) && n_rows <= kMcWgCapacity && n_cols_local == n_rows &&
           plan.n_halo() == 0;
}

// The format of colouring c.  The host counts rows and entries per colour (which
// colours take a wave per row, where the slices start); the row list (a stable sort by colour),
// the slice widths and offsets and the cells are built on the device from one upload of the
// rows in local | halo column numbering.
void DevMatrix::build_mc_gs(Colouring&& cin, uint64_t seed) {
    AMG_CHECK(square, "multicolour GS needs a square matrix");
    AMG_CHECK(!ctx->capturing, "multicolour GS: format requested inside a graph capture");
    const HostCSR& H = host_image();
    const int n = (int)n_rows;
    AMG_CHECK((int64_t)cin.colour.size() == n_rows, "multicolour GS: one colour per local row");
    hipStream_t s = ctx->stream;
    McGsFormat f;
    f.colouring = std::move(cin);
    f.seed = seed;
    const std::vector<int32_t>& colour = f.colouring.colour;
    const int nc = f.colouring.n_colours;
    std::vector<int64_t> crow((size_t)nc + 1, 0), cnz((size_t)nc, 0);
    for (int i = 0; i < n; ++i) {
        AMG_CHECK(colour[i] >= 0 && colour[i] < nc, "multicolour GS: colour out of range");
        ++crow[(size_t)colour[i] + 1];
        cnz[colour[i]] += H.rp[i + 1] - H.rp[i];
    }
    for (int c = 0; c < nc; ++c) crow[c + 1] += crow[c];
    f.cslice_host.assign((size_t)nc + 1, 0);
    f.wave_host.assign((size_t)std::max(nc, 1), 0);
    std::vector<int2> span;
    std::vector<uint8_t> swave;
    for (int c = 0; c < nc; ++c) {
        const int64_t rows_c = crow[c + 1] - crow[c];
        const bool wv = rows_c > 0 && cnz[c] > (int64_t)kMcSlice * rows_c;
        f.wave_host[c] = wv;
        const int step = wv ? 1 : 64;
        for (int64_t p = crow[c]; p < crow[c + 1]; p += step) {
            span.push_back(make_int2((int)p, (int)std::min<int64_t>(step, crow[c + 1] - p)));
            swave.push_back(wv);
        }
        f.cslice_host[c + 1] = (int)span.size();
    }
    const int ns = f.n_slices = (int)span.size();
    f.cslice.upload(f.cslice_host.data(), f.cslice_host.size());
    f.wave.upload(f.wave_host.data(), f.wave_host.size());
    f.rows.alloc((size_t)std::max(n, 1));
    f.dinv.alloc((size_t)std::max(n, 1));
    f.slices.alloc((size_t)std::max(ns, 1));
    if (n > 0) {
        // the rows as the level kernels number their columns: local ids, then the halo's
        hvec<int> lc((size_t)std::max<int64_t>(nnz, 1));
        const int64_t c0 = first_col, c1 = first_col + n_cols_local;
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < nnz; ++k) {
            const int64_t g = H.col[k];
            lc[k] = g >= c0 && g < c1 ? (int)(g - c0) : (int)(n_cols_local + plan.find(g));
        }
        DevBuf<int> ccol, dcolour, iota, skey, width, cells, off;
        DevBuf<double> cval;
        DevBuf<int2> dspan;
        DevBuf<uint8_t> dswave;
        DevBuf<char> tmp;
        ccol.upload(lc.data(), lc.size());
        cval.upload(H.val.data(), (size_t)std::max<int64_t>(nnz, 1));
        dcolour.upload(colour.data(), (size_t)n);
        dspan.upload(span.data(), span.size());
        dswave.upload(swave.data(), swave.size());
        iota.alloc((size_t)n);
        skey.alloc((size_t)n);
        hipLaunchKernelGGL(mc_iota_kernel, dim3(grid_of(n, kTPB)), dim3(kTPB), 0, s, n, iota.p);
        int bits = 1;
        while (bits < 31 && (1ll << bits) < nc) ++bits;
        size_t bytes = 0;
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, dcolour.p, skey.p, iota.p, f.rows.p, n, 0, bits, s));
        tmp.alloc(std::max<size_t>(bytes, 1));
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, dcolour.p, skey.p, iota.p, f.rows.p, n, 0, bits, s));
        width.alloc((size_t)ns + 1);
        cells.alloc((size_t)ns + 1);
        off.alloc((size_t)ns + 1);
        HIP_CHECK(hipMemsetAsync(cells.p, 0, sizeof(int) * cells.n, s));
        hipLaunchKernelGGL(mc_width_kernel, dim3(grid_of(ns, kTPB)), dim3(kTPB), 0, s, ns, dspan.p, dswave.p, f.rows.p,
                           rp.p, width.p, cells.p);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, cells.p, off.p, ns + 1, s));
        if (tmp.n < bytes) tmp.alloc(bytes);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, cells.p, off.p, ns + 1, s));
        int total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, off.p + ns, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        f.cells = (int64_t)total * 64;
        AMG_CHECK(total >= 0 && f.cells < INT_MAX, "multicolour GS: format exceeds int32 indexing");
        f.col.alloc((size_t)std::max<int64_t>(f.cells, 1));
        f.val.alloc((size_t)std::max<int64_t>(f.cells, 1));
        hipLaunchKernelGGL(mc_fill_kernel, dim3(grid_of(ns, kTPB / 64)), dim3(kTPB), 0, s, ns, dspan.p, dswave.p,
                           f.rows.p, rp.p, ccol.p, cval.p, dinv.p, width.p, off.p, f.slices.p, f.col.p, f.val.p,
                           f.dinv.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));  // the build's buffers are freed here
    } else {
        f.col.alloc(1);
        f.val.alloc(1);
    }
    // one sweep: the cells' columns and values, the slice headers, per row its list entry, 1 / a_ii,
    // b and the x it writes, and x (local and halo) read once
    f.bytes = 12 * f.cells + 16 * (int64_t)ns + 28 * n_rows + 8 * (n_cols_local + plan.n_halo());
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(mc_gs_wg_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       kMcWgCapacity * (int)sizeof(double));
    HIP_CHECK(attr);
    f.built = true;
    mc = std::move(f);
    ++format_generation;  // captured cycles hold the old format's pointers
}

void par_mc_gs(DevMatrix& A, double* x, const double* b, bool backward, int path) {
    AMG_CHECK(A.mc.built, "multicolour GS: the operator has no colouring (amg_par_csr_colour)");
    AMG_CHECK(path >= 0 && path <= 2, "multicolour GS: path must be 0, 1 or 2");
    const bool fits = A.mc_one_wg_fits();
    AMG_CHECK(path != 2 || fits,
              "multicolour GS: the one-workgroup sweep takes an operator without a halo exchange of at most " +
                  std::to_string(kMcWgCapacity) + " rows");
    const McGsFormat& f = A.mc;
    hipStream_t s = A.ctx->stream;
    const int nc = f.colouring.n_colours;
    McArgs a{f.slices.p, f.rows.p, f.col.p, f.val.p, f.dinv.p, b, x, A.halo.p, (int)A.n_cols_local};
    if (path == 2 || (path == 0 && fits && A.n_rows <= mc_wg_rows())) {
        if (A.n_rows == 0) return;
        hipLaunchKernelGGL(mc_gs_wg_kernel, dim3(1), dim3(kMcWgThreads), (size_t)A.n_rows * sizeof(double), s, a,
                           f.cslice.p, f.wave.p, nc, (int)A.n_rows, backward ? 1 : 0);
        HIP_CHECK(hipGetLastError());
        return;
    }
    for (int t = 0; t < nc; ++t) {
        const int c = backward ? nc - 1 - t : t;
        // every rank walks every colour: the exchange is collective, rows of the colour or not
        if (A.halo_begin(x)) A.halo_wait();
        const int s0 = f.cslice_host[c], s1 = f.cslice_host[c + 1];
        if (s1 == s0) continue;
        const dim3 grid(grid_of(s1 - s0, kTPB / 64));
        if (f.wave_host[c]) hipLaunchKernelGGL(mc_gs_colour_kernel<true>, grid, dim3(kTPB), 0, s, a, s0, s1);
        else hipLaunchKernelGGL(mc_gs_colour_kernel<false>, grid, dim3(kTPB), 0, s, a, s0, s1);
        HIP_CHECK(hipGetLastError());
    }
}

}  // namespace amg
