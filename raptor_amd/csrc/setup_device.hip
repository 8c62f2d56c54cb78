// setup_device.hip -- AMG setup on the GPU: strength of connection,
// PMIS splitting, classical and extended+i interpolation, MIS(2) aggregation and the
// smoothed-aggregation prolongator on any number of ranks, the transpose R = P^T on one
// rank.  Every integer decision and every floating-point sum follows host_setup.cpp /
// oracle/amg_oracle.c exactly, so the hierarchy is bit-identical to the host
// path's at every rank count; the Galerkin products stay on the device SpGEMM (spgemm.hip).
//
// Layout: one upload of this rank's rows of A per level -- int32 row_ptr, int32 GLOBAL column
// ids, fp64 values; the strength graph S stays on the device; per-row kernels are one thread
// per row (rows are short and independent); rounds (PMIS, MIS(2)) are synchronous: each round
// reads the previous round's states only, other ranks' states through a halo (Dist) that is
// forwarded between rounds (device pack, host setup exchange, upload).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "device.hpp"

namespace amg {

namespace {

enum { ST_U = -1, ST_F = 0, ST_C = 1 };
enum { M_OUT = 0, M_U = 1, M_IN = 2 };
constexpr int kT = 256;

inline unsigned grid1(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

__device__ __forceinline__ unsigned long long dmix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// host_comm.cpp hash32()
__device__ __forceinline__ unsigned dhash32(long long gid, unsigned long long seed) {
    return (unsigned)(dmix((unsigned long long)gid ^ (seed * 0x9E3779B97F4A7C15ull)) >> 32);
}

// binary search of c in the ascending cols[lo, hi)
__device__ __forceinline__ int dfind(const int* cols, int lo, int hi, int c) {
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        const int v = cols[m];
        if (v == c) return m;
        if (v < c) lo = m + 1;
        else hi = m;
    }
    return -1;
}

// rows of this rank: local row i is global row lo + i; columns are GLOBAL ids (int32: the
// global size is checked < 2^31), ascending per row -- the host image's order, so every
// loop below visits entries exactly as host_setup.cpp does
struct DCsr {
    const int* rp;
    const int* col;
    const double* val;
    int n;
    int lo;
};

// where the state of global point g lives: local rows [lo, lo + n) or the sorted halo ids
// gid[0, nh) (several ranks: states forwarded from their owners each round)
struct Dist {
    int lo, n;
    const int* gid;
    int nh;
    // >= 0: local index; < 0: halo index -(t + 1); INT_MIN: neither
    __device__ __forceinline__ int loc(int g) const {
        if (g >= lo && g < lo + n) return g - lo;
        int a = 0, b = nh;
        while (a < b) {
            const int m = (a + b) >> 1;
            const int v = gid[m];
            if (v == g) return -m - 1;
            if (v < g) a = m + 1;
            else b = m;
        }
        return INT_MIN;
    }
    template <class T>
    __device__ __forceinline__ T get(const T* local, const T* halo, int g) const {
        const int l = loc(g);
        return l >= 0 ? local[l] : halo[-l - 1];
    }
};

// ---- strength ------------------------------------------------------------------------
// classical: m_i = max_{j != i} (-a_ij) (first entry sets it); none if m_i <= 0;
// strong iff -a_ij >= theta m_i.  Pass 0 counts, pass 1 fills (row order kept).
template <bool FILL>
__global__ void strength_classical_kernel(DCsr A, double theta, int* cnt, const int* srp, int* scol,
                                          double* sval) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= A.n) return;
    double mx = 0.0;
    bool any = false;
    const int gi = A.lo + i;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        if (A.col[k] == gi) continue;
        const double v = -A.val[k];
        if (!any || v > mx) mx = v;
        any = true;
    }
    const bool has = any && mx > 0.0;
    const double thr = theta * mx;
    int q = FILL ? srp[i] : 0, c = 0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        if (!(has && A.col[k] != gi && -A.val[k] >= thr)) continue;
        if (FILL) {
            scol[q] = A.col[k];
            sval[q++] = A.val[k];
        }
        ++c;
    }
    if (!FILL) cnt[i] = c;
}

// a_ii: the first diagonal entry of the row (0 if none), like diagonal()
__global__ void diagonal_kernel(DCsr A, double* d) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= A.n) return;
    double v = 0.0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
        if (A.col[k] == A.lo + i) {
            v = A.val[k];
            break;
        }
    d[i] = v;
}

// SA strength, signed (r6; host_setup.cpp sa_strong): -a_ij >= theta sqrt(|a_ii a_jj|), j != i
// (a_jj of another rank's column through D: the forwarded diagonal hd)
__device__ __forceinline__ bool dsa_strong(double aij, double di, double dj, double theta) {
    return -aij >= theta * sqrt(fabs(di * dj));
}

template <bool FILL>
__global__ void strength_symmetric_kernel(DCsr A, Dist D, const double* d, const double* hd, double theta,
                                          int* cnt, const int* srp, int* scol, double* sval) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= A.n) return;
    int q = FILL ? srp[i] : 0, c = 0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int j = A.col[k];
        if (j == A.lo + i) continue;
        if (!dsa_strong(A.val[k], d[i], D.get(d, hd, j), theta)) continue;
        if (FILL) {
            scol[q] = j;
            sval[q++] = A.val[k];
        }
        ++c;
    }
    if (!FILL) cnt[i] = c;
}

// ---- PMIS ------------------------------------------------------------------------------
// |S^T_i| over this rank's rows: local columns only (off-rank dependents arrive as pairs)
__global__ void col_count_kernel(DCsr S, int* tcnt) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
        const int c = S.col[k] - S.lo;
        if (c >= 0 && c < S.n) atomicAdd(&tcnt[c], 1);
    }
}

// S^T adjacency of the local-local part (row j of S^T = the global ids of local rows i with
// j in S_i; order within a row arbitrary -- PMIS only takes maxima over the set)
__global__ void transpose_fill_kernel(DCsr S, int* cursor, int* tcol) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
        const int c = S.col[k] - S.lo;
        if (c >= 0 && c < S.n) tcol[atomicAdd(&cursor[c], 1)] = S.lo + i;
    }
}

// entries of S whose column lives on another rank: (column, dependent row) pairs, row order
template <bool FILL>
__global__ void offrank_kernel(DCsr S, int* cnt, const int* orp, int* pc, int* pj) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    int q = FILL ? orp[i] : 0, c = 0;
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
        const int g = S.col[k];
        if (g >= S.lo && g < S.lo + S.n) continue;
        if (FILL) {
            pc[q] = g;
            pj[q++] = S.lo + i;
        }
        ++c;
    }
    if (!FILL) cnt[i] = c;
}

// key = |S^T_i| << 32 | hash32(global id): tcnt = local dependents, ecnt = off-rank ones
__global__ void pmis_init_kernel(int n, int lo, const int* tcnt, const int* erp, unsigned long long seed,
                                 unsigned long long* key, int* cf) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int c = tcnt[i] + (erp ? erp[i + 1] - erp[i] : 0);
    key[i] = ((unsigned long long)c << 32) | (unsigned long long)dhash32(lo + i, seed);
    cf[i] = c == 0 ? ST_F : ST_U;
}

// undecided i -> C iff its (key, global id) beats every undecided j in S_i u S^T_i (local
// dependents tcol, off-rank dependents ecol); halo states / keys through D
__global__ void pmis_select_kernel(DCsr S, Dist D, const int* trp, const int* tcol, const int* erp,
                                   const int* ecol, const unsigned long long* key,
                                   const unsigned long long* hkey, const int* cf, const int* hcf,
                                   unsigned char* newc) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    newc[i] = 0;
    if (cf[i] != ST_U) return;
    const unsigned long long ki = key[i];
    const int gi = S.lo + i;
    bool best = true;
    auto beats = [&](int g) {  // false when undecided neighbour g outranks i
        const int l = D.loc(g);
        const int sj = l >= 0 ? cf[l] : hcf[-l - 1];
        if (sj != ST_U) return true;
        const unsigned long long kj = l >= 0 ? key[l] : hkey[-l - 1];
        return !(kj > ki || (kj == ki && g > gi));
    };
    for (int k = S.rp[i]; k < S.rp[i + 1] && best; ++k) best = beats(S.col[k]);
    for (int t = trp[i]; t < trp[i + 1] && best; ++t) best = beats(tcol[t]);
    if (erp)
        for (int t = erp[i]; t < erp[i + 1] && best; ++t) best = beats(ecol[t]);
    newc[i] = best;
}

__global__ void pmis_apply_kernel(int n, const unsigned char* newc, int* cf) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n && newc[i]) cf[i] = ST_C;
}

// undecided i with a C point in S_i -> F; count the undecided that remain
__global__ void pmis_fpass_kernel(DCsr S, Dist D, int* cf, const int* hcf, unsigned long long* nu) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n || cf[i] != ST_U) return;
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k)
        if (D.get(cf, hcf, S.col[k]) == ST_C) {
            cf[i] = ST_F;
            return;
        }
    atomicAdd(nu, 1ull);
}

// ---- multicolour ordering ---------------------------------------------------
// key = hash32(global id); u precedes v iff key(u) > key(v), or the keys tie and u < v
__global__ void colour_init_kernel(int n, int lo, unsigned long long seed, unsigned* key, int* colour) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    key[i] = dhash32(lo + i, seed);
    colour[i] = -1;
}

// One readiness round of the first-fit colouring on the pattern of A u A^T (rows of A, local
// dependents tcol, off-rank dependents ecol; the diagonal and repeated neighbours are harmless):
// an uncoloured row whose preceding neighbours are all coloured takes the smallest colour none
// of them uses (64 colours per pass over its neighbours).  Reads the previous round's colours
// only; newc[i] = the colour taken, -1: not this round
__global__ void colour_select_kernel(DCsr A, Dist D, const int* trp, const int* tcol, const int* erp,
                                     const int* ecol, const unsigned* key, const unsigned* hkey, const int* colour,
                                     const int* hcolour, int* newc) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= A.n) return;
    newc[i] = -1;
    if (colour[i] >= 0) return;
    const unsigned ki = key[i];
    const int gi = A.lo + i;
    // colour of neighbour g if it precedes i (-1: uncoloured), -2 if it does not precede
    auto before = [&](int g) {
        if (g == gi) return -2;
        const int l = D.loc(g);
        const unsigned kj = l >= 0 ? key[l] : hkey[-l - 1];
        if (!(kj > ki || (kj == ki && g < gi))) return -2;
        return l >= 0 ? colour[l] : hcolour[-l - 1];
    };
    bool ready = true;
    for (int k = A.rp[i]; k < A.rp[i + 1] && ready; ++k) ready = before(A.col[k]) != -1;
    for (int t = trp[i]; t < trp[i + 1] && ready; ++t) ready = before(tcol[t]) != -1;
    if (erp)
        for (int t = erp[i]; t < erp[i + 1] && ready; ++t) ready = before(ecol[t]) != -1;
    if (!ready) return;
    for (int base = 0;; base += 64) {
        unsigned long long used = 0;
        auto take = [&](int g) {
            const int c = before(g) - base;
            if (c >= 0 && c < 64) used |= 1ull << c;
        };
        for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) take(A.col[k]);
        for (int t = trp[i]; t < trp[i + 1]; ++t) take(tcol[t]);
        if (erp)
            for (int t = erp[i]; t < erp[i + 1]; ++t) take(ecol[t]);
        if (~used) {
            newc[i] = base + __ffsll((long long)~used) - 1;
            return;
        }
    }
}

// colours taken this round become visible; counts the rows still uncoloured and the largest colour
__global__ void colour_apply_kernel(int n, const int* newc, int* colour, unsigned long long* left, int* cmax) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    if (newc[i] >= 0) {
        colour[i] = newc[i];
        atomicMax(cmax, newc[i]);
    } else if (colour[i] < 0) {
        atomicAdd(left, 1ull);
    }
}

// halo forwarding: packed[t] = local[send_idx[t]]
template <class T>
__global__ void pack_kernel_t(int n, const int* idx, const T* local, T* packed) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t < n) packed[t] = local[idx[t]];
}

// ---- classical interpolation ------------------------------------------------------------
// is global j a strong neighbour of local row i (S rows ascending)
__device__ __forceinline__ bool strong(const DCsr& S, int i, int j) {
    return dfind(S.col, S.rp[i], S.rp[i + 1], j) >= 0;
}

// rows of A reachable from this rank: local rows, and the ghost rows of the halo points
// (D's halo = A's off-rank columns; ghost row t of halo point D.gid[t], global column ids)
struct ARows {
    DCsr A;
    Dist D;
    const int* grp;
    const int* gcol;
    const double* gval;
    __device__ __forceinline__ void row(int g, int& b, int& e, const int*& c, const double*& v) const {
        const int l = D.loc(g);
        if (l >= 0) {
            b = A.rp[l], e = A.rp[l + 1], c = A.col, v = A.val;
        } else {
            const int t = -l - 1;
            b = grp[t], e = grp[t + 1], c = gcol, v = gval;
        }
    }
};

// F row i: d = a_ii + weak couplings + couplings to strong F neighbours whose s_k is 0;
// w_ij = -num_j / d for j in C_i (strong C neighbours), num_j = a_ij + sum over strong F
// neighbours k (A-row order) of (a_ik a_kj) / s_k, s_k = sum of row k's couplings to C_i of
// sign opposite to a_kk.  Same loops and order as host_setup.cpp interp_classical().
// cf / cmap of halo points through R.D (hcf, hcmap); P columns are global coarse ids.
template <bool FILL>
__device__ void interp_row_serial(const ARows& R, const DCsr& S, const int* cf, const int* hcf, const int* cmap,
                                  const int* hcmap, int* cnt, const int* prp, int* pcol, double* pval, int i) {
    const DCsr& A = R.A;
    if (cf[i] == ST_C) {
        if (FILL) {
            pcol[prp[i]] = cmap[i];
            pval[prp[i]] = 1.0;
        } else {
            cnt[i] = 1;
        }
        return;
    }
    const int gi = A.lo + i;
    // strong first: a strong neighbour is a column of row i, so its state is local or halo
    auto is_c = [&](int g) { return R.D.get(cf, hcf, g) == ST_C; };
    auto in_ci = [&](int m) { return m != gi && strong(S, i, m) && is_c(m); };
    double d = 0.0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
        if (A.col[k] == gi) {
            d = A.val[k];
            break;
        }
    int nci = 0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int j = A.col[k];
        if (j == gi) continue;
        const bool st = strong(S, i, j);
        if (st && is_c(j)) ++nci;
        else if (!st) d += A.val[k];
    }
    if (!FILL) {
        cnt[i] = nci;
        return;
    }
    if (nci == 0) return;
    // s_k of strong F neighbour kk over its row (local or ghost)
    auto s_of = [&](int kk, bool& pos) {
        int b, e;
        const int* rc;
        const double* rv;
        R.row(kk, b, e, rc, rv);
        double akk = 0.0;
        for (int u = b; u < e; ++u)
            if (rc[u] == kk) {
                akk = rv[u];
                break;
            }
        pos = akk > 0.0;
        double s = 0.0;
        for (int u = b; u < e; ++u) {
            const double v = rv[u];
            if ((pos ? v < 0.0 : v > 0.0) && in_ci(rc[u])) s += v;
        }
        return s;
    };
    // s_k == 0 neighbours add a_ik to d, in A-row order (second pass of the host loop)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int kk = A.col[k];
        if (kk == gi || !strong(S, i, kk) || is_c(kk)) continue;
        bool pos;
        if (s_of(kk, pos) == 0.0) d += A.val[k];
    }
    // num_j accumulates in this row's own P slots (pval), k outer: s_k is formed once per
    // strong F neighbour instead of once per (j, k) pair, and every num_j still receives its
    // terms in A-row order of k -- the host loop's order, so the weights are bit-identical
    const int q0 = prp[i];
    int q = q0;
    for (int kj = A.rp[i]; kj < A.rp[i + 1]; ++kj) {
        const int j = A.col[kj];
        if (j == gi || !strong(S, i, j) || !is_c(j)) continue;
        pcol[q] = R.D.get(cmap, hcmap, j);
        pval[q++] = A.val[kj];
    }
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int kk = A.col[k];
        if (kk == gi || !strong(S, i, kk) || is_c(kk)) continue;
        bool pos;
        const double s = s_of(kk, pos);
        if (s == 0.0) continue;
        int b, e;
        const int* rc;
        const double* rv;
        R.row(kk, b, e, rc, rv);
        q = q0;
        for (int kj = A.rp[i]; kj < A.rp[i + 1]; ++kj) {
            const int j = A.col[kj];
            if (j == gi || !strong(S, i, j) || !is_c(j)) continue;
            const int uj = dfind(rc, b, e, j);
            if (uj >= 0 && (pos ? rv[uj] < 0.0 : rv[uj] > 0.0)) pval[q] += (A.val[k] * rv[uj]) / s;
            ++q;
        }
    }
    for (q = q0; q < q0 + nci; ++q) pval[q] = -pval[q] / d;
}

template <bool FILL>
__global__ void interp_kernel(ARows R, DCsr S, const int* cf, const int* hcf, const int* cmap,
                              const int* hcmap, int* cnt, const int* prp, int* pcol, double* pval) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < R.A.n) interp_row_serial<FILL>(R, S, cf, hcf, cmap, hcmap, cnt, prp, pcol, pval, i);
}

// Wave-per-row form of interp_kernel for operators with long rows (the Galerkin levels: a
// thread per row walked 50-100-entry rows and their neighbours' rows serially, 13-52 ms per
// launch on grids of 3-4,249 workgroups).  The same sums in the same order:
//  * lanes classify the row's entries (strong / C / diagonal) into LDS and form s_k of the
//    strong F neighbours, one neighbour per lane (s_k's own loop is serial, as in s_of);
//  * lane 0 forms d in the host's two passes (weak couplings in row order, then the strong F
//    neighbours with s_k == 0 in row order);
//  * lane q forms num_j of the q-th strong C neighbour: a_ij, then + (a_ik a_kj) / s_k over the
//    strong F neighbours k in row order -- one accumulator per lane, the host's k order.
// Rows longer than kIwMax entries run interp_kernel's loops on lane 0.
constexpr int kIwWaves = 4, kIwMax = 512;
enum { IW_STRONG = 1, IW_C = 2, IW_DIAG = 4, IW_POS = 8 };

template <bool FILL>
__global__ __launch_bounds__(64 * kIwWaves) void interp_wave_kernel(ARows R, DCsr S, const int* cf, const int* hcf,
                                                                    const int* cmap, const int* hcmap, int* cnt,
                                                                    const int* prp, int* pcol, double* pval) {
    __shared__ unsigned char fl_s[kIwWaves][kIwMax];
    __shared__ double sv_s[kIwWaves][kIwMax];
    const DCsr& A = R.A;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kIwWaves + w;
    if (i >= A.n) return;  // wave-uniform
    unsigned char* fl = fl_s[w];
    double* sv = sv_s[w];
    const int b0 = A.rp[i], e0 = A.rp[i + 1], len = e0 - b0;
    if (cf[i] == ST_C || len > kIwMax) {
        if (lane == 0) interp_row_serial<FILL>(R, S, cf, hcf, cmap, hcmap, cnt, prp, pcol, pval, i);
        return;
    }
    const int gi = A.lo + i;
    auto is_c = [&](int g) { return R.D.get(cf, hcf, g) == ST_C; };
    auto in_ci = [&](int m) { return m != gi && strong(S, i, m) && is_c(m); };
    // entry classes; nci = strong C neighbours
    int nci = 0;
    for (int k0 = 0; k0 < len; k0 += 64) {
        const int k = k0 + lane;
        unsigned char f = 0;
        if (k < len) {
            const int j = A.col[b0 + k];
            if (j == gi) {
                f = IW_DIAG;
            } else if (strong(S, i, j)) {
                f = IW_STRONG | (is_c(j) ? IW_C : 0);
            }
            fl[k] = f;
        }
        nci += __popcll(__ballot(f == (IW_STRONG | IW_C)));
    }
    if (!FILL) {
        if (lane == 0) cnt[i] = nci;
        return;
    }
    if (nci == 0) return;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // s_k of the strong F neighbours (interp_kernel's s_of), one per lane
    for (int k0 = 0; k0 < len; k0 += 64) {
        const int k = k0 + lane;
        if (k < len && fl[k] == IW_STRONG) {
            const int kk = A.col[b0 + k];
            int b, e;
            const int* rc;
            const double* rv;
            R.row(kk, b, e, rc, rv);
            double akk = 0.0;
            for (int u = b; u < e; ++u)
                if (rc[u] == kk) {
                    akk = rv[u];
                    break;
                }
            const bool pos = akk > 0.0;
            double sk = 0.0;
            for (int u = b; u < e; ++u) {
                const double v = rv[u];
                if ((pos ? v < 0.0 : v > 0.0) && in_ci(rc[u])) sk += v;
            }
            sv[k] = sk;
            if (pos) fl[k] = IW_STRONG | IW_POS;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // d: a_ii (first diagonal entry), + weak couplings in row order, + strong F with s_k == 0
    double d = 0.0;
    if (lane == 0) {
        for (int k = 0; k < len; ++k)
            if (fl[k] & IW_DIAG) {
                d = A.val[b0 + k];
                break;
            }
        for (int k = 0; k < len; ++k)
            if (fl[k] == 0) d += A.val[b0 + k];
        for (int k = 0; k < len; ++k)
            if ((fl[k] & (IW_STRONG | IW_C)) == IW_STRONG && sv[k] == 0.0) d += A.val[b0 + k];
    }
    d = __shfl(d, 0, 64);
    // num_j, lane = strong C neighbour (q order = row order)
    const int q0 = prp[i];
    int qbase = 0;
    for (int k0 = 0; k0 < len; k0 += 64) {
        const int kj = k0 + lane;
        const bool isc = kj < len && fl[kj] == (IW_STRONG | IW_C);
        const unsigned long long m = __ballot(isc);
        if (isc) {
            const int q = qbase + __popcll(m & ((1ull << lane) - 1ull));
            const int j = A.col[b0 + kj];
            double num = A.val[b0 + kj];
            for (int k = 0; k < len; ++k) {
                const unsigned char f = fl[k];
                if ((f & (IW_STRONG | IW_C)) != IW_STRONG) continue;
                const double sk = sv[k];
                if (sk == 0.0) continue;
                const int kk = A.col[b0 + k];
                int b, e;
                const int* rc;
                const double* rv;
                R.row(kk, b, e, rc, rv);
                const int uj = dfind(rc, b, e, j);
                const bool pos = (f & IW_POS) != 0;
                if (uj >= 0 && (pos ? rv[uj] < 0.0 : rv[uj] > 0.0)) num += (A.val[b0 + k] * rv[uj]) / sk;
            }
            pcol[q0 + q] = R.D.get(cmap, hcmap, j);
            pval[q0 + q] = -num / d;
        }
        qbase += __popcll(m);
    }
}

// ---- extended+i interpolation -----------------------------------------------------------
// host_setup.cpp interp_ext_i(), one wavefront per F row:
//  * gather: the C members of S_i and of S_k for every strong F neighbour k (local k: its S
//    row; ghost k: the classical strength test recomputed from the ghost row) go into a hash
//    set, which drops duplicates as they arrive; the set is compacted and rank-sorted into the
//    ascending list C^_i (ascending fine ids = ascending coarse ids);
//  * the count pass ends there: min(|C^_i|, p_max) entries;
//  * s_k: one strong neighbour per lane, a serial sum in row k's order;
//  * d: lane 0, the host's order (a_ii, the weak entries outside C^_i in row order, the strong
//    F neighbours in row order);
//  * num_j: one member of C^_i per lane: a_ij, then (a_ik a_kj) / s_k in row order of k;
//  * truncation: lane 0 runs the host's loops on the weights in LDS.
// The set, the list, s_k and the weights live in LDS (kExtCap members and kExtCap strong
// neighbours per wave).  A row with more of either is listed in the count pass and runs the
// same code with its tables in global scratch sized from the row's own bound (ExtSlot).
// State lookups go through D2, the halo of ext_state_plan() (two deep); rows through R.
constexpr int kExtWaves = 4, kExtCap = 256, kExtTab = 2 * kExtCap;
enum { EX_F = 1, EX_POS = 2 };

struct ExtArgs {
    ARows R;
    DCsr S;
    Dist D2;
    const int* cf;
    const int* hcf;
    const int* cmap;
    const int* hcmap;
    double theta;
    int p_max;
    int* cnt;
    const int* prp;
    int* pcol;
    double* pval;
    unsigned char* ovf;  // per row: runs the scratch path
    int* ovf_list;       // rows flagged by the count pass, ovf_n[0] of them
    int* ovf_n;
    int* err;            // a scratch table filled up (cannot happen: sized from the row's bound)
    int row0;            // first row of this launch (launches are chunked: kExtLaunchRows)
};

// an overflow row's tables in global scratch: T hash slots (a power of two), T / 2 list members
struct ExtSlot {
    long long io, dof, bo;  // offsets into the int / double / byte scratch
    int row, T, slen;
};

// Orders one wave's table writes before its other lanes' reads.  The tables are private to the
// wave.  In LDS nothing more is needed.  In the scratch form (global memory) the plain stores
// and loads of raw / lst / sk / fl / w rely on a wave's own stores being visible to its later
// loads through the CU's vector L1 (write-through, one L1 per CU: the default, non-split
// mode), so a wavefront-scope fence is enough; only the hash set, which is written with
// atomics that go to L2, is read back with an agent-scope atomic load.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// 1: g claimed an empty slot, 0: already there, -1: no slot left after T probes.
// T is a power of two >= 128: the home slot is the top log2(T) bits of the product
__device__ __forceinline__ int ext_insert(int* tab, int T, int g) {
    unsigned h = ((unsigned)g * 0x9E3779B1u) >> (__clz(T) + 1);
    for (int p = 0; p < T; ++p) {
        const int old = atomicCAS(&tab[h], -1, g);
        if (old == -1) return 1;
        if (old == g) return 0;
        h = (h + 1) & (unsigned)(T - 1);
    }
    return -1;
}

// One F row.  tab[T] (all -1 on entry), raw[cap], lst[cap], sk[scap], w[cap], fl[max(cap, scap)];
// w may alias tab (the set is dead once compacted).  Returns false if the row does not fit
// (nothing written); GLOBAL: the tables are global memory (the set is read back past the L1).
template <bool FILL, bool GLOBAL>
__device__ bool ext_row(const ExtArgs& a, int i, int lane, int* tab, int T, int* raw, int* lst, int cap, double* sk,
                        int scap, double* w, unsigned char* fl) {
    const DCsr& A = a.R.A;
    const DCsr& S = a.S;
    const int gi = A.lo + i;
    const int sb = S.rp[i], slen = S.rp[i + 1] - sb;
    if (slen > scap) return false;
    // a candidate is a column of a local or a ghost row: local or in D2's halo (else: err)
    auto is_c = [&](int g) {
        const int l = a.D2.loc(g);
        if (l == INT_MIN) {
            atomicExch(a.err, 1);
            return false;
        }
        return (l >= 0 ? a.cf[l] : a.hcf[-l - 1]) == ST_C;
    };
    int m = 0;
    bool full = false;
    // one batch of candidates, a lane each (called by the whole wave)
    auto batch = [&](bool valid, int g) {
        int r = 0;
        if (valid && is_c(g)) r = ext_insert(tab, T, g);
        m += __popcll(__ballot(r == 1));
        if (__ballot(r < 0)) full = true;
    };
    for (int t0 = 0; t0 < slen; t0 += 64) {
        const int t = t0 + lane;
        batch(t < slen, t < slen ? S.col[sb + t] : 0);
        if (m > cap || full) return false;
    }
    for (int t = 0; t < slen; ++t) {
        const int k = S.col[sb + t];  // wave-uniform
        if (is_c(k)) continue;
        const int l = a.R.D.loc(k);
        if (l >= 0) {
            const int b = S.rp[l], e = S.rp[l + 1];
            for (int u0 = b; u0 < e; u0 += 64) {
                const int u = u0 + lane;
                batch(u < e, u < e ? S.col[u] : 0);
                if (m > cap || full) return false;
            }
        } else {
            // ghost row: strength_classical's test, the maximum over the lanes (exact)
            const int tt = -l - 1, b = a.R.grp[tt], e = a.R.grp[tt + 1];
            double mx = 0.0;
            bool any = false;
            for (int u = b + lane; u < e; u += 64) {
                if (a.R.gcol[u] == k) continue;
                const double v = -a.R.gval[u];
                if (!any || v > mx) mx = v;
                any = true;
            }
            for (int off = 32; off; off >>= 1) {
                const double omx = __shfl_xor(mx, off, 64);
                const bool oany = __shfl_xor((int)any, off, 64) != 0;
                if (oany && (!any || omx > mx)) mx = omx;
                any = any || oany;
            }
            const bool has = any && mx > 0.0;
            const double thr = a.theta * mx;
            for (int u0 = b; u0 < e; u0 += 64) {
                const int u = u0 + lane;
                const bool ok = u < e && has && a.R.gcol[u] != k && -a.R.gval[u] >= thr;
                batch(ok, ok ? a.R.gcol[u] : 0);
                if (m > cap || full) return false;
            }
        }
    }
    if (!FILL) {
        if (lane == 0) a.cnt[i] = a.p_max > 0 && m > a.p_max ? a.p_max : m;
        return true;
    }
    if (m == 0) return true;
    // the set, compacted and sorted by rank (members are distinct)
    wave_sync();
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int g = GLOBAL ? __hip_atomic_load(&tab[t0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             : tab[t0 + lane];
        const unsigned long long mask = __ballot(g != -1);
        if (g != -1) raw[base + __popcll(mask & ((1ull << lane) - 1ull))] = g;
        base += __popcll(mask);
    }
    wave_sync();
    for (int q = lane; q < m; q += 64) {
        const int g = raw[q];
        int r = 0;
        for (int x = 0; x < m; ++x) r += raw[x] < g;
        lst[r] = g;
    }
    wave_sync();
    // s_k of the strong F neighbours, one per lane; row k's order
    for (int t = lane; t < slen; t += 64) {
        const int k = S.col[sb + t];
        unsigned char f = 0;
        double s = 0.0;
        if (!is_c(k)) {
            int b, e;
            const int* rc;
            const double* rv;
            a.R.row(k, b, e, rc, rv);
            double akk = 0.0;
            for (int u = b; u < e; ++u)
                if (rc[u] == k) {
                    akk = rv[u];
                    break;
                }
            const bool pos = akk > 0.0;
            for (int u = b; u < e; ++u) {
                const double v = rv[u];
                if ((pos ? v < 0.0 : v > 0.0) && (rc[u] == gi || dfind(lst, 0, m, rc[u]) >= 0)) s += v;
            }
            f = EX_F | (pos ? EX_POS : 0);
        }
        sk[t] = s;
        fl[t] = f;
    }
    wave_sync();
    // d on lane 0, the host's order
    const int b0 = A.rp[i], e0 = A.rp[i + 1];
    double d = 0.0;
    if (lane == 0) {
        for (int k = b0; k < e0; ++k)
            if (A.col[k] == gi) {
                d = A.val[k];
                break;
            }
        for (int k = b0; k < e0; ++k) {
            const int j = A.col[k];
            if (j == gi || dfind(lst, 0, m, j) >= 0 || strong(S, i, j)) continue;
            d += A.val[k];
        }
        for (int t = 0; t < slen; ++t) {
            const unsigned char f = fl[t];
            if (!(f & EX_F)) continue;
            const double aik = S.val[sb + t];
            if (sk[t] == 0.0) {
                d += aik;
                continue;
            }
            int b, e;
            const int* rc;
            const double* rv;
            a.R.row(S.col[sb + t], b, e, rc, rv);
            const int u = dfind(rc, b, e, gi);
            if (u >= 0 && ((f & EX_POS) ? rv[u] < 0.0 : rv[u] > 0.0)) d += (aik * rv[u]) / sk[t];
        }
    }
    d = __shfl(d, 0, 64);
    // w_j, one member of C^_i per lane
    const bool trunc = a.p_max > 0 && m > a.p_max;
    const int q0 = a.prp[i];
    for (int q = lane; q < m; q += 64) {
        const int j = lst[q];
        double num = 0.0;
        const int uij = dfind(A.col, b0, e0, j);
        if (uij >= 0) num += A.val[uij];
        for (int t = 0; t < slen; ++t) {
            const unsigned char f = fl[t];
            if (!(f & EX_F)) continue;
            const double s = sk[t];
            if (s == 0.0) continue;
            int b, e;
            const int* rc;
            const double* rv;
            a.R.row(S.col[sb + t], b, e, rc, rv);
            const int u = dfind(rc, b, e, j);
            if (u >= 0 && ((f & EX_POS) ? rv[u] < 0.0 : rv[u] > 0.0)) num += (S.val[sb + t] * rv[u]) / s;
        }
        const double wq = -num / d;
        if (trunc) {
            w[q] = wq;
        } else {
            a.pcol[q0 + q] = a.D2.get(a.cmap, a.hcmap, j);
            a.pval[q0 + q] = wq;
        }
    }
    if (!trunc) return true;
    wave_sync();
    // P_max truncation: the host's loops (sums from 0.0 in ascending column order; the larger
    // |w| wins, ties to the smaller column); fl now marks the kept members
    if (lane == 0) {
        double tot = 0.0, kept = 0.0;
        for (int q = 0; q < m; ++q) tot += w[q], fl[q] = 0;
        for (int r = 0; r < a.p_max; ++r) {
            int best = -1;
            for (int q = 0; q < m; ++q)
                if (!fl[q] && (best < 0 || fabs(w[q]) > fabs(w[best]))) best = q;
            fl[best] = 1;
        }
        for (int q = 0; q < m; ++q)
            if (fl[q]) kept += w[q];
        const double f = kept != 0.0 ? tot / kept : 0.0;
        int o = q0;
        for (int q = 0; q < m; ++q) {
            if (!fl[q]) continue;
            a.pcol[o] = a.D2.get(a.cmap, a.hcmap, lst[q]);
            a.pval[o++] = kept != 0.0 ? w[q] * f : w[q];
        }
    }
    return true;
}

template <bool FILL>
__global__ __launch_bounds__(64 * kExtWaves) void interp_ext_kernel(ExtArgs a) {
    __shared__ double wt_s[kExtWaves][kExtCap];  // the hash set (kExtTab ints), then the weights
    __shared__ int raw_s[kExtWaves][kExtCap], lst_s[kExtWaves][kExtCap];
    __shared__ double sk_s[kExtWaves][kExtCap];
    __shared__ unsigned char fl_s[kExtWaves][kExtCap];
    static_assert(kExtTab * sizeof(int) == kExtCap * sizeof(double), "the weights reuse the set's storage");
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = a.row0 + blockIdx.x * kExtWaves + wv;
    if (i >= a.R.A.n) return;  // wave-uniform
    if (a.cf[i] == ST_C) {
        if (lane == 0) {
            if (FILL) {
                a.pcol[a.prp[i]] = a.cmap[i];
                a.pval[a.prp[i]] = 1.0;
            } else {
                a.cnt[i] = 1;
            }
        }
        return;
    }
    if (FILL && a.ovf[i]) return;
    int* tab = reinterpret_cast<int*>(wt_s[wv]);
    for (int t = lane; t < kExtTab; t += 64) tab[t] = -1;
    wave_sync();
    const bool ok = ext_row<FILL, false>(a, i, lane, tab, kExtTab, raw_s[wv], lst_s[wv], kExtCap, sk_s[wv], kExtCap,
                                         wt_s[wv], fl_s[wv]);
    if (!FILL && !ok && lane == 0) {
        a.ovf[i] = 1;
        a.cnt[i] = 0;
        a.ovf_list[atomicAdd(a.ovf_n, 1)] = i;
    }
}

// the rows the LDS form listed, a wave each, tables in global scratch (iscr preset to -1)
template <bool FILL>
__global__ __launch_bounds__(64 * kExtWaves) void interp_ext_scratch_kernel(ExtArgs a, const ExtSlot* slots, int nslots,
                                                                            int* iscr, double* dscr,
                                                                            unsigned char* bscr) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * kExtWaves + wv;
    if (r >= nslots) return;
    const ExtSlot sl = slots[r];
    const int cap = sl.T / 2;
    int* tab = iscr + sl.io;
    const bool ok = ext_row<FILL, true>(a, sl.row, lane, tab, sl.T, tab + sl.T, tab + sl.T + cap, cap,
                                        dscr + sl.dof + cap, sl.slen, dscr + sl.dof, bscr + sl.bo);
    if (!ok && lane == 0) atomicExch(a.err, 1);
}

// ---- MIS(2) aggregation -----------------------------------------------------------------
// tuple (state, hash, global id) of every local point, packed hi = state << 32 | hash, lo = id
__global__ void mis2_tuple_kernel(int n, int lo, const int* st, const unsigned* hs, unsigned long long* h,
                                  unsigned long long* l) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    h[i] = ((unsigned long long)(unsigned)st[i] << 32) | hs[i];
    l[i] = (unsigned long long)(lo + i);
}

// one hop of the lexicographic max over S_i (halo tuples through D: hh / hl)
__global__ void mis2_hop_kernel(DCsr S, Dist D, const unsigned long long* h0, const unsigned long long* l0,
                                const unsigned long long* hh, const unsigned long long* hl,
                                unsigned long long* h1, unsigned long long* l1) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    unsigned long long mh = h0[i], ml = l0[i];
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
        const int l = D.loc(S.col[k]);
        const unsigned long long xh = l >= 0 ? h0[l] : hh[-l - 1], xl = l >= 0 ? l0[l] : hl[-l - 1];
        if (xh > mh || (xh == mh && xl > ml)) mh = xh, ml = xl;
    }
    h1[i] = mh;
    l1[i] = ml;
}

__global__ void mis2_update_kernel(int n, int lo, const unsigned long long* h, const unsigned long long* l,
                                   int* st, unsigned long long* nu) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n || st[i] != M_U) return;
    if (l[i] == (unsigned long long)(lo + i)) st[i] = M_IN;
    else if ((h[i] >> 32) == M_IN) st[i] = M_OUT;
    if (st[i] == M_U) atomicAdd(nu, 1ull);
}

// pass 1: a root keeps its aggregate id (aggr: the global id of a root, -1 otherwise); the
// others join the first root neighbour in S-row order
__global__ void mis2_pass1_kernel(DCsr S, Dist D, const int* aggr, const int* haggr, int* a1) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    int a = aggr[i];
    if (a < 0)
        for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
            const int aj = D.get(aggr, haggr, S.col[k]);
            if (aj >= 0) {
                a = aj;
                break;
            }
        }
    a1[i] = a;
}

// pass 2: the rest join the pass-1 neighbour with max |s_ij| (ties: smaller aggregate id)
__global__ void mis2_pass2_kernel(DCsr S, Dist D, const int* a1, const int* ha1, int* agg,
                                  unsigned long long* orphans) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= S.n) return;
    if (a1[i] >= 0) {
        agg[i] = a1[i];
        return;
    }
    double best = -1.0;
    int ba = -1;
    for (int k = S.rp[i]; k < S.rp[i + 1]; ++k) {
        const int aj = D.get(a1, ha1, S.col[k]);
        if (aj < 0) continue;
        const double w = fabs(S.val[k]);
        if (w > best || (w == best && aj < ba)) best = w, ba = aj;
    }
    agg[i] = ba;
    if (ba < 0) atomicAdd(orphans, 1ull);
}

// ---- SA smoothing (r6; host_setup.cpp sa_filter / sa_rho / sa_prolongator) ------------------
// the filtered operator: the diagonal and the strong off-diagonals in row order; the diagonal
// value f_i = a_ii + the weak off-diagonals (row order).  Pass 0 counts, pass 1 fills.
template <bool FILL>
__global__ void sa_filter_kernel(DCsr A, Dist D, const double* d, const double* hd, double theta, int* cnt,
                                 const int* frp, int* fcol, double* fval) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= A.n) return;
    const int gi = A.lo + i;
    if (!FILL) {
        int c = 0;
        for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
            const int j = A.col[k];
            c += j == gi || dsa_strong(A.val[k], d[i], D.get(d, hd, j), theta);
        }
        cnt[i] = c;
        return;
    }
    double f = d[i];
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int j = A.col[k];
        if (j != gi && !dsa_strong(A.val[k], d[i], D.get(d, hd, j), theta)) f += A.val[k];
    }
    int q = frp[i];
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
        const int j = A.col[k];
        if (j == gi) {
            fcol[q] = j;
            fval[q++] = f;
        } else if (dsa_strong(A.val[k], d[i], D.get(d, hd, j), theta)) {
            fcol[q] = j;
            fval[q++] = A.val[k];
        }
    }
}

__global__ void max_abs_kernel(int n, const double* __restrict__ x, unsigned long long* m) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n) dmax_abs(m, x[i]);
}

__global__ void div_scalar_kernel(int n, const double* __restrict__ y, double lam, double* __restrict__ x) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n) x[i] = y[i] / lam;
}

// one power step: y_i = (A_F x)_i / a_ii (row order from 0.0), max |y_i|
__global__ void sa_power_kernel(DCsr F, Dist D, const double* __restrict__ x, const double* __restrict__ hx,
                                const double* __restrict__ d, double* __restrict__ y, unsigned long long* m) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= F.n) return;
    double s = 0.0;
    for (int k = F.rp[i]; k < F.rp[i + 1]; ++k) s += F.val[k] * D.get(x, hx, F.col[k]);
    const double v = s / d[i];
    y[i] = v;
    dmax_abs(m, v);
}

// P = T - (omega / a_ii) (A_F T): row i's products (agg_k, f_ik t_k) in A_F's row order,
// insertion-sorted by aggregate (stable: row order kept inside an aggregate) into the row's
// slice of the scratch; pass 0 sorts and counts the distinct aggregates with T's (agg_i);
// pass 1 sums each aggregate's products from 0.0 in that order and merges T's entry
template <bool FILL>
__global__ void sa_smooth_kernel(DCsr F, Dist D, const int* __restrict__ agg, const int* __restrict__ hagg,
                                 const double* __restrict__ t, const double* __restrict__ ht,
                                 const double* __restrict__ d, double omega, int* __restrict__ skey,
                                 double* __restrict__ sval, long long* __restrict__ cnt,
                                 const long long* __restrict__ prp, long long* __restrict__ pcol,
                                 double* __restrict__ pval) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= F.n) return;
    const int b = F.rp[i], e = F.rp[i + 1], ai = agg[i];
    if (!FILL) {
        for (int k = b; k < e; ++k) {
            const int g = F.col[k];
            const int key = D.get(agg, hagg, g);
            const double v = F.val[k] * D.get(t, ht, g);
            int p = k;
            while (p > b && skey[p - 1] > key) {
                skey[p] = skey[p - 1];
                sval[p] = sval[p - 1];
                --p;
            }
            skey[p] = key;
            sval[p] = v;
        }
        long long c = 0;
        bool tin = false;
        for (int k = b; k < e; ++k) {
            if (k == b || skey[k] != skey[k - 1]) ++c;
            tin = tin || skey[k] == ai;
        }
        cnt[i] = c + (tin ? 0 : 1);
        return;
    }
    const double c = omega * (1.0 / d[i]);
    long long q = prp[i];
    bool tleft = true;
    int k = b;
    while (k < e || tleft) {
        const long long ja = k < e ? (long long)skey[k] : LLONG_MAX, jj = tleft ? (long long)ai : LLONG_MAX;
        const long long j = ja < jj ? ja : jj;
        double tvv = 0.0, av = 0.0;
        if (jj == j) {
            tvv = t[i];
            tleft = false;
        }
        if (ja == j)
            for (; k < e && skey[k] == j; ++k) av += sval[k];
        pcol[q] = j;
        pval[q++] = tvv - c * av;
    }
}

// MIS(2) roots: flags for the exclusive scan that numbers them, then each root's aggregate id
__global__ void root_flag_kernel(int n, const int* st, int* flag) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n) flag[i] = st[i] == M_IN;
}

__global__ void root_id_kernel(int n, const int* st, const int* pos, int base, int* aggr) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n) aggr[i] = st[i] == M_IN ? base + pos[i] : -1;
}

// ---- transpose: R = P^T, rows of R sorted by fine index (stable radix sort on columns) ---
__global__ void iota_kernel(int n, int* v) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < n) v[i] = i;
}

__global__ void expand_rows_kernel(const int* rp, int n, int* rowof) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    for (int k = rp[i]; k < rp[i + 1]; ++k) rowof[k] = i;
}

__global__ void gather_transpose_kernel(int nnz, const int* perm, const int* rowof, const double* val,
                                        long long* rcol, double* rval) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t >= nnz) return;
    const int k = perm[t];
    rcol[t] = rowof[k];
    rval[t] = val[k];
}

__global__ void count_cols_kernel(int nnz, const int* col, int* cnt) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t < nnz) atomicAdd(&cnt[col[t]], 1);
}

// N ranks: the transpose's exchange record (the host transpose's layout: R row j, R column i
// = global fine row, value)
struct TRec {
    long long j, i;
    double v;
};

// send side: entries in (column, fine row) order -- the radix sort by column is stable over
// the row-major entry order -- as records; the owner of column j receives a contiguous range
__global__ void transpose_records_kernel(int nnz, const int* __restrict__ keys, const int* __restrict__ perm,
                                        const int* __restrict__ rowof, const double* __restrict__ val,
                                        long long i0, TRec* __restrict__ out) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t >= nnz) return;
    const int k = perm[t];
    out[t] = TRec{keys[t], i0 + rowof[k], val[k]};
}

// receive side: the local row of every record (j - lo), the key of a stable sort that keeps
// rank order, then ascending i, inside each row
__global__ void record_rows_kernel(int m, const TRec* __restrict__ in, long long lo, int* __restrict__ key) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t < m) key[t] = (int)(in[t].j - lo);
}

__global__ void gather_records_kernel(int m, const int* __restrict__ perm, const TRec* __restrict__ in,
                                      long long* __restrict__ rcol, double* __restrict__ rval) {
    const int t = blockIdx.x * kT + threadIdx.x;
    if (t >= m) return;
    const TRec e = in[perm[t]];
    rcol[t] = e.i;
    rval[t] = e.v;
}

// first sorted position with key >= bound[o], per owner boundary o
__global__ void owner_bounds_kernel(int m, const int* __restrict__ keys, int nb, const long long* __restrict__ bound,
                                    long long* __restrict__ out) {
    const int o = blockIdx.x * kT + threadIdx.x;
    if (o >= nb) return;
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)keys[mid] < bound[o]) lo = mid + 1;
        else hi = mid;
    }
    out[o] = lo;
}

// ---- helpers ---------------------------------------------------------------------------
// one thread per row.  Nothing is launched for n == 0 -- only the launch is skipped: a rank
// without rows still makes every collective call around it
template <class K, class... Args>
void launch_rows(hipStream_t s, long long n, K kernel, Args... args) {
    if (n == 0) return;
    hipLaunchKernelGGL(kernel, dim3(grid1(n)), dim3(kT), 0, s, args...);
    HIP_CHECK(hipGetLastError());
}

// one device word, once the stream has produced it
template <class T>
T read_scalar(hipStream_t s, const T* dev) {
    T v{};
    HIP_CHECK(hipMemcpyAsync(&v, dev, sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return v;
}

// exclusive scan of n ints / long longs into out[0..n]; returns out[n], the total
template <class I>
int64_t exclusive_scan(hipStream_t s, const I* in, I* out, int n, DevBuf<char>& tmp) {
    size_t bytes = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n + 1, s));
    if (tmp.n < bytes) tmp.alloc(bytes);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, n + 1, s));
    return read_scalar(s, out + n);
}

std::vector<int32_t> download_ints(hipStream_t s, const int* p, int64_t n) {
    std::vector<int32_t> h((size_t)n);
    copy_to_host(h.data(), p, sizeof(int) * n, s);
    return h;
}

// index-width conversions of the setup's device images (grid-stride: up to 2^31 entries)
__global__ void narrow_kernel(long long n, const long long* __restrict__ in, int* __restrict__ out) {
    for (long long t = (long long)blockIdx.x * kT + threadIdx.x; t < n; t += (long long)gridDim.x * kT)
        out[t] = (int)in[t];
}

__global__ void widen_kernel(long long n, const int* __restrict__ in, long long* __restrict__ out) {
    for (long long t = (long long)blockIdx.x * kT + threadIdx.x; t < n; t += (long long)gridDim.x * kT)
        out[t] = in[t];
}

inline unsigned grid_cap(long long n) { return std::min<unsigned>(grid1(n), 1u << 16); }

}  // namespace

void DevCsr::ensure_rp32(hipStream_t s) {
    if (rp32.p) return;
    AMG_CHECK(rp64.p && nnz < INT_MAX, "device image: row pointers exceed int32 indexing");
    rp32.alloc((size_t)n + 1);
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_cap(n + 1)), dim3(kT), 0, s, (long long)n + 1, rp64.p, rp32.p);
    HIP_CHECK(hipGetLastError());
}

void DevCsr::ensure_rp64(hipStream_t s) {
    if (rp64.p) return;
    AMG_CHECK(rp32.p, "device image without row pointers");
    rp64.alloc((size_t)n + 1);
    hipLaunchKernelGGL(widen_kernel, dim3(grid_cap(n + 1)), dim3(kT), 0, s, (long long)n + 1, rp32.p, rp64.p);
    HIP_CHECK(hipGetLastError());
}

void DevCsr::ensure_col32(hipStream_t s) {
    if (col32.p) return;
    AMG_CHECK(col64.p && ncols < INT_MAX, "device image: columns exceed int32 indexing");
    col32.alloc((size_t)std::max<int64_t>(nnz, 1));
    if (nnz)
        hipLaunchKernelGGL(narrow_kernel, dim3(grid_cap(nnz)), dim3(kT), 0, s, (long long)nnz, col64.p, col32.p);
    HIP_CHECK(hipGetLastError());
}

void DevCsr::ensure_col64(hipStream_t s) {
    if (col64.p) return;
    AMG_CHECK(col32.p, "device image without columns");
    col64.alloc((size_t)std::max<int64_t>(nnz, 1));
    if (nnz)
        hipLaunchKernelGGL(widen_kernel, dim3(grid_cap(nnz)), dim3(kT), 0, s, (long long)nnz, col32.p, col64.p);
    HIP_CHECK(hipGetLastError());
}

DevCsr* SetupImages::find(const HostCSR& M) {
    for (auto& kv : e)
        if (kv.first == M.rp.data() && kv.second->n == M.nrows() && kv.second->nnz == M.nnz()) return kv.second.get();
    return nullptr;
}

DevCsr& SetupImages::get(const HostCSR& M) {
    if (DevCsr* d = find(M)) return *d;
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 columns");
    std::unique_ptr<DevCsr> d(new DevCsr());
    d->rp64.upload(reinterpret_cast<const long long*>(M.rp.data()), M.rp.size());
    if (M.nnz()) {
        d->col64.upload(reinterpret_cast<const long long*>(M.col.data()), (size_t)M.nnz());
        d->val.upload(M.val.data(), (size_t)M.nnz());
    } else {
        d->col64.alloc(1);
        d->val.alloc(1);
    }
    DevCsr& r = *d;
    put(M, std::move(d));
    return r;
}

void SetupImages::put(const HostCSR& M, std::unique_ptr<DevCsr> d) {
    d->n = M.nrows();
    d->nnz = M.nnz();
    d->ncols = M.n_global_cols;
    for (auto& kv : e)
        if (kv.first == M.rp.data()) {
            kv.second = std::move(d);
            return;
        }
    e.emplace_back(M.rp.data(), std::move(d));
}

void SetupImages::keep_only(const HostCSR& M) {
    std::vector<std::pair<const int64_t*, std::unique_ptr<DevCsr>>> keep;
    for (auto& kv : e)
        if (kv.first == M.rp.data()) keep.push_back(std::move(kv));
    e.swap(keep);
}

namespace {

// coarse drop tolerance on the device (one rank: global column = local row).  d_i = the row's
// stored diagonal (first match, 0.0 without one: then nothing of the row is dropped)
__global__ void sp_diag_kernel(long long n, const long long* __restrict__ rp, const long long* __restrict__ col,
                               const double* __restrict__ val, double* __restrict__ d) {
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        double v = 0.0;
        for (long long k = rp[i]; k < rp[i + 1]; ++k)
            if (col[k] == i) {
                v = val[k];
                break;
            }
        d[i] = v;
    }
}

__device__ __forceinline__ bool sp_dropped(long long i, long long j, double v, const double* d, double tau) {
    return j != i && fabs(v) < tau * sqrt(fabs(d[i] * d[j]));
}

// FILL = false: kept entries per row; true: the kept entries in row order, the diagonal's value
// a_ii + the dropped entries of the row (row order) -- host sparsify's loop
template <bool FILL>
__global__ void sp_rows_kernel(long long n, const long long* __restrict__ rp, const long long* __restrict__ col,
                               const double* __restrict__ val, const double* __restrict__ d, double tau,
                               int* __restrict__ cnt, const int* __restrict__ orp, long long* __restrict__ ocol,
                               double* __restrict__ oval) {
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        if (!FILL) {
            int c = 0;
            for (long long k = rp[i]; k < rp[i + 1]; ++k) c += sp_dropped(i, col[k], val[k], d, tau) ? 0 : 1;
            cnt[i] = c;
            continue;
        }
        double f = d[i];
        for (long long k = rp[i]; k < rp[i + 1]; ++k)
            if (sp_dropped(i, col[k], val[k], d, tau)) f += val[k];
        long long o = orp[i];
        for (long long k = rp[i]; k < rp[i + 1]; ++k) {
            const long long j = col[k];
            if (sp_dropped(i, j, val[k], d, tau)) continue;
            ocol[o] = j;
            oval[o] = j == i ? f : val[k];
            ++o;
        }
    }
}

}  // namespace

HostCSR sparsify_device(Context& ctx, const HostComm& comm, const HostCSR& A, double tau, SetupImages* imgs) {
    DevCsr* D = imgs && comm.nranks == 1 ? imgs->find(A) : nullptr;
    if (!D || A.nrows() >= INT_MAX || A.nnz() >= INT_MAX) return sparsify(comm, A, tau);  // int32 scan
    hipStream_t s = ctx.stream;
    D->ensure_rp64(s);
    D->ensure_col64(s);
    const int64_t n = A.nrows();
    DevBuf<double> d;
    DevBuf<int> cnt, orp;
    DevBuf<char> tmp;
    d.alloc((size_t)std::max<int64_t>(n, 1));
    cnt.alloc((size_t)n + 1);
    orp.alloc((size_t)n + 1);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int) * cnt.n, s));
    if (n) {
        hipLaunchKernelGGL(sp_diag_kernel, dim3(grid_cap(n)), dim3(kT), 0, s, (long long)n, D->rp64.p, D->col64.p,
                           D->val.p, d.p);
        hipLaunchKernelGGL(sp_rows_kernel<false>, dim3(grid_cap(n)), dim3(kT), 0, s, (long long)n, D->rp64.p,
                           D->col64.p, D->val.p, d.p, tau, cnt.p, nullptr, nullptr, nullptr);
        HIP_CHECK(hipGetLastError());
    }
    const int64_t nnz = exclusive_scan(s, cnt.p, orp.p, (int)n, tmp);
    std::unique_ptr<DevCsr> B(new DevCsr());
    B->rp32 = std::move(orp);
    B->col64.alloc((size_t)std::max<int64_t>(nnz, 1));
    B->val.alloc((size_t)std::max<int64_t>(nnz, 1));
    if (n)
        hipLaunchKernelGGL(sp_rows_kernel<true>, dim3(grid_cap(n)), dim3(kT), 0, s, (long long)n, D->rp64.p, D->col64.p,
                           D->val.p, d.p, tau, nullptr, B->rp32.p, B->col64.p, B->val.p);
    HIP_CHECK(hipGetLastError());
    HostCSR out;
    out.n_global_rows = A.n_global_rows;
    out.n_global_cols = A.n_global_cols;
    out.row_starts = A.row_starts;
    out.col_starts = A.col_starts;
    std::vector<int> hrp = download_ints(s, B->rp32.p, n + 1);
    out.rp.assign(hrp.begin(), hrp.end());
    out.col.resize((size_t)nnz);
    out.val.resize((size_t)nnz);
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 columns");
    copy_to_host(out.col.data(), B->col64.p, sizeof(long long) * nnz, s);
    copy_to_host(out.val.data(), B->val.p, sizeof(double) * nnz, nullptr);
    imgs->put(out, std::move(B));
    return out;
}

namespace {

// Setup state that is built in place and passed by reference, never copied or moved: the
// kernels' argument structs (Dist, ARows, ExtArgs) hold raw pointers into these buffers, and
// later stages keep pointers to the plans and ghost rows
struct Pinned {
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
};

// what every stage of one level reads: this rank's rows of A on the host and on the device
struct LevelCtx : Pinned {
    hipStream_t s;
    const HostComm& comm;
    const HostCSR& A;
    const amg_options& opt;
    const int level, n, lo;
    const bool dist;
    PhaseTimer tm;
    DCsr Av{};          // A's device image (int32 rows, global column ids)
    DevBuf<char> tmp;   // the scans' scratch
    LevelCtx(hipStream_t stream, const HostComm& c, const HostCSR& Ah, const amg_options& o, int l)
        : s(stream), comm(c), A(Ah), opt(o), level(l), n((int)Ah.nrows()), lo((int)Ah.row_starts[c.rank]),
          dist(c.nranks > 1), tm(c) {}
    uint64_t seed() const { return opt.seed + (uint64_t)level; }
};

// CSR rows built on the device by a count and a fill pass: the strength graph, SA's filtered
// operator (int, global column ids) and P (int: PMIS, long long: SA)
template <class I>
struct DevRows : Pinned {
    DevBuf<I> rp, col;
    DevBuf<double> val;
    int64_t nnz = 0;
};
using DevS = DevRows<int>;
DCsr view(const LevelCtx& L, const DevS& M) { return DCsr{M.rp.p, M.col.p, M.val.p, L.n, L.lo}; }

// count(cnt) writes a count per row, the exclusive scan of the counts is rp[0..n], fill(rp, total)
// allocates what it fills from the total and writes each row at its offset; returns the total
template <class I, class CountK, class FillK>
int64_t count_scan_fill(hipStream_t s, int n, DevBuf<I>& rp, DevBuf<char>& tmp, CountK count, FillK fill) {
    DevBuf<I> cnt;
    cnt.alloc((size_t)n + 1);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(I) * cnt.n, s));
    count(cnt.p);
    rp.alloc((size_t)n + 1);
    const int64_t total = exclusive_scan(s, cnt.p, rp.p, n, tmp);
    fill(rp.p, total);
    HIP_CHECK(hipGetLastError());
    return total;
}

// the same for CSR rows: fill(rp, col, val)
template <class I, class CountK, class FillK>
void build_rows_with(LevelCtx& L, DevRows<I>& M, CountK count, FillK fill) {
    M.nnz = count_scan_fill(L.s, L.n, M.rp, L.tmp, count, [&](const I* rp, int64_t nnz) {
        M.col.alloc((size_t)std::max<int64_t>(nnz, 1));
        M.val.alloc((size_t)std::max<int64_t>(nnz, 1));
        fill(rp, M.col.p, M.val.p);
    });
}

// ... by a thread-per-row kernel pair K<false> (counts) / K<true> (fills) whose parameters are
// lead..., then (cnt, rp, col, val)
template <class I, class KC, class KF, class... Lead>
void build_rows(LevelCtx& L, DevRows<I>& M, KC count_k, KF fill_k, Lead... lead) {
    build_rows_with(
        L, M, [&](I* cnt) { launch_rows(L.s, L.n, count_k, lead..., cnt, nullptr, nullptr, nullptr); },
        [&](const I* rp, I* col, double* val) { launch_rows(L.s, L.n, fill_k, lead..., nullptr, rp, col, val); });
}

// A halo on the device: its plan, the sorted global ids (Dist lookups), the local send indices,
// and forward(): pack on the device, the setup exchange on the host, the halo values uploaded.
// forward() is collective: every rank of a distributed level calls it, rows or not
struct DevHalo : Pinned {
    HaloPlan plan;
    DevBuf<int> gid, sidx;
    void build(HaloPlan p) {
        plan = std::move(p);
        std::vector<int> g(plan.halo_gid.begin(), plan.halo_gid.end()), si(plan.send_idx.begin(), plan.send_idx.end());
        gid.upload(g.data(), g.size());
        sidx.upload(si.data(), si.size());
    }
    Dist dist(int lo, int n) const { return Dist{lo, n, gid.p, (int)plan.n_halo()}; }
    template <class T>
    void forward(hipStream_t s, const HostComm& comm, const T* local, DevBuf<T>& halo) const {
        const HaloPlan& p = plan;
        const int ns = (int)p.send_idx.size();
        DevBuf<T> packed;
        packed.alloc((size_t)std::max(ns, 1));
        launch_rows(s, ns, pack_kernel_t<T>, ns, sidx.p, local, packed.p);
        std::vector<T> sbuf((size_t)ns), rbuf((size_t)p.n_halo());
        if (ns) HIP_CHECK(hipMemcpyAsync(sbuf.data(), packed.p, sizeof(T) * ns, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::vector<int64_t> sb(comm.nranks, 0), rb(comm.nranks, 0);
        for (size_t q = 0; q < p.send_procs.size(); ++q)
            sb[p.send_procs[q]] = (p.send_ptr[q + 1] - p.send_ptr[q]) * (int64_t)sizeof(T);
        for (size_t q = 0; q < p.recv_procs.size(); ++q)
            rb[p.recv_procs[q]] = (p.recv_ptr[q + 1] - p.recv_ptr[q]) * (int64_t)sizeof(T);
        comm.alltoallv(sbuf.data(), sb, rbuf.data(), rb);
        if (halo.n < rbuf.size() || halo.n == 0) halo.alloc(std::max<size_t>(rbuf.size(), 1));
        if (!rbuf.empty())
            HIP_CHECK(hipMemcpyAsync(halo.p, rbuf.data(), sizeof(T) * rbuf.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

// Extended+i on the device (interp_ext_kernel): init() forwards cf and the coarse ids through
// the two-deep state halo, count() fills the row counts, fill() the entries.  Rows the LDS form
// lists in count() run interp_ext_scratch_kernel in both passes, in batches whose scratch
// stays under kExtScratchInts.
constexpr int64_t kExtScratchInts = int64_t(1) << 26;  // 256 MiB of hash slots and lists per batch
constexpr int kExtLaunchRows = 1 << 18;                // rows (wavefronts) per interp_ext_kernel launch
static_assert(kExtLaunchRows % kExtWaves == 0, "a launch covers whole workgroups of rows");

struct ExtInterp : Pinned {
    hipStream_t s = nullptr;
    const HostCSR* A = nullptr;  // A, its halo plan and ghost rows: the level's, which outlive this
    const HaloPlan* aplan = nullptr;
    const GhostRows* G = nullptr;
    DevHalo SH;
    DevBuf<int> scf, scmap, olist, on, err, iscr;
    DevBuf<unsigned char> ovf, bscr;
    DevBuf<double> dscr;
    ExtArgs a{};
    int n = 0, lo = 0, nc_global = 0;
    int launches = 0;             // count-pass launches of the LDS form
    std::vector<ExtSlot> slots;   // the rows of the scratch path

    void init(hipStream_t stream, const HostComm& comm, const HostCSR& Ah, const HaloPlan& ap, const GhostRows& Gh,
              const ARows& Ar, const DCsr& Sv, const int* cf, const int* cmap, int ncg, const amg_options& opt) {
        s = stream, A = &Ah, aplan = &ap, G = &Gh;
        n = Ar.A.n, lo = Ar.A.lo, nc_global = ncg;
        SH.build(comm.nranks > 1 ? ext_state_plan(comm, Ah, ap, Gh) : HaloPlan());
        scf.alloc(1);
        scmap.alloc(1);
        if (comm.nranks > 1) {
            SH.forward(s, comm, cf, scf);
            SH.forward(s, comm, cmap, scmap);
        }
        const size_t nn = (size_t)std::max(n, 1);
        ovf.alloc(nn);
        olist.alloc(nn);
        on.alloc(1);
        err.alloc(1);
        HIP_CHECK(hipMemsetAsync(ovf.p, 0, nn, s));
        HIP_CHECK(hipMemsetAsync(on.p, 0, sizeof(int), s));
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(int), s));
        a.R = Ar, a.S = Sv, a.D2 = SH.dist(lo, n);
        a.cf = cf, a.hcf = scf.p, a.cmap = cmap, a.hcmap = scmap.p;
        a.theta = opt.strong_threshold, a.p_max = opt.p_max;
        a.cnt = nullptr, a.prp = nullptr, a.pcol = nullptr, a.pval = nullptr;
        a.ovf = ovf.p, a.ovf_list = olist.p, a.ovf_n = on.p, a.err = err.p;
    }

    // length of row g of A: a local row or a ghost row of A's halo
    int64_t row_len(int64_t g) const {
        if (g >= lo && g < lo + n) return A->rp[g - lo + 1] - A->rp[g - lo];
        const int64_t h = aplan->find(g);
        return G->rp[h + 1] - G->rp[h];
    }

    // the listed rows' tables: |C^_i| <= min(sum of the row lengths of row i's columns, all C)
    void plan_slots() {
        const int no = read_scalar(s, on.p);
        if (!no) return;
        std::vector<int32_t> rows = download_ints(s, olist.p, no);
        std::sort(rows.begin(), rows.end());
        for (int32_t i : rows) {
            int64_t ub = 0;
            for (int64_t k = A->rp[i]; k < A->rp[i + 1]; ++k) ub += row_len(A->col[k]);
            ub = std::min<int64_t>(std::max<int64_t>(ub, A->rp[i + 1] - A->rp[i]), std::max(nc_global, 1));
            int64_t T = 128;
            while (T < 2 * ub) T *= 2;
            AMG_CHECK(T < INT_MAX, "device setup: extended+i row exceeds int32 indexing");
            slots.push_back(ExtSlot{0, 0, 0, i, (int)T, (int)(A->rp[i + 1] - A->rp[i])});
        }
    }

    template <bool FILL>
    void run_slots() {
        for (size_t c0 = 0; c0 < slots.size();) {
            size_t c1 = c0;
            int64_t ni = 0, nd = 0, nb = 0;
            while (c1 < slots.size() && (c1 == c0 || ni + 2 * (int64_t)slots[c1].T <= kExtScratchInts)) {
                ExtSlot& sl = slots[c1++];
                sl.io = ni, sl.dof = nd, sl.bo = nb;
                ni += 2 * (int64_t)sl.T;
                nd += sl.T / 2 + sl.slen;
                nb += sl.T / 2 + sl.slen;
            }
            if (iscr.n < (size_t)ni) iscr.alloc((size_t)ni);
            if (dscr.n < (size_t)nd) dscr.alloc((size_t)nd);
            if (bscr.n < (size_t)nb) bscr.alloc((size_t)nb);
            HIP_CHECK(hipMemsetAsync(iscr.p, 0xFF, sizeof(int) * (size_t)ni, s));
            DevBuf<ExtSlot> ds;
            ds.upload(slots.data() + c0, c1 - c0);
            const int ns = (int)(c1 - c0);
            hipLaunchKernelGGL(interp_ext_scratch_kernel<FILL>, dim3((unsigned)((ns + kExtWaves - 1) / kExtWaves)),
                               dim3(64 * kExtWaves), 0, s, a, ds.p, ns, iscr.p, dscr.p, bscr.p);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));  // ds and the batch's scratch are reused
            c0 = c1;
        }
    }

    // a wave per row: 64 n threads pass the 2^32 threads of one grid dimension from n = 2^26 rows
    // on (7-pt 512^3 on one rank), so the rows go in launches of kExtLaunchRows (as spgemm.hip
    // chunks its row kernels); returns the number of launches
    template <bool FILL>
    int launch_waves() {
        int launches = 0;
        for (int64_t r0 = 0; r0 < n; r0 += kExtLaunchRows, ++launches) {
            const int rows = (int)std::min<int64_t>(kExtLaunchRows, n - r0);
            a.row0 = (int)r0;
            hipLaunchKernelGGL(interp_ext_kernel<FILL>, dim3((unsigned)((rows + kExtWaves - 1) / kExtWaves)),
                               dim3(64 * kExtWaves), 0, s, a);
            HIP_CHECK(hipGetLastError());
        }
        a.row0 = 0;
        return launches;
    }

    void count(int* cnt) {
        a.cnt = cnt;
        launches = launch_waves<false>();
        plan_slots();
        run_slots<false>();
    }

    void fill(const int* prp, int* pcol, double* pval) {
        a.cnt = nullptr, a.prp = prp, a.pcol = pcol, a.pval = pval;
        launch_waves<true>();
        run_slots<true>();
        const int e = read_scalar(s, err.p);
        AMG_ASSERT(e == 0);
    }
};

// ---- PMIS level: the stages of pmis_level ---------------------------------------------------
void classical_strength(LevelCtx& L, DevS& S) {
    build_rows(L, S, strength_classical_kernel<false>, strength_classical_kernel<true>, L.Av, L.opt.strong_threshold);
}

// several ranks: off-rank dependents (pairs (i, j), j on another rank depends on local i) as the
// rows erp / ecol, and the halo plan of the neighbourhoods S_i u S^T_i, as pmis_split builds them
HaloPlan offrank_dependents(LevelCtx& L, const DCsr& Sv, DevBuf<int>& erp, DevBuf<int>& ecol) {
    const HostComm& comm = L.comm;
    const int n = L.n, lo = L.lo;
    DevBuf<int> orp, opc, opj;
    const int64_t no = count_scan_fill(
        L.s, n, orp, L.tmp,
        [&](int* cnt) { launch_rows(L.s, n, offrank_kernel<false>, Sv, cnt, nullptr, nullptr, nullptr); },
        [&](const int* rp, int64_t total) {
            opc.alloc((size_t)std::max<int64_t>(total, 1));
            opj.alloc((size_t)std::max<int64_t>(total, 1));
            launch_rows(L.s, n, offrank_kernel<true>, Sv, nullptr, rp, opc.p, opj.p);
        });
    const std::vector<int32_t> pc = download_ints(L.s, opc.p, no), pj = download_ints(L.s, opj.p, no);
    std::vector<std::vector<int64_t>> sendp(comm.nranks);
    std::vector<int64_t> need;
    for (int64_t t = 0; t < no; ++t) {
        const int o = owner_of(L.A.col_starts, pc[t]);
        sendp[o].push_back(pc[t]);
        sendp[o].push_back(pj[t]);
        need.push_back(pc[t]);
    }
    const auto gotp = comm.exchange(sendp);
    std::vector<int> ec((size_t)n + 1, 0);
    for (int r = 0; r < comm.nranks; ++r)
        for (size_t t = 0; t < gotp[r].size(); t += 2) ++ec[gotp[r][t] - lo + 1];
    for (int i = 0; i < n; ++i) ec[i + 1] += ec[i];
    std::vector<int> el((size_t)std::max(ec[n], 1)), pos(ec.begin(), ec.end() - 1);
    for (int r = 0; r < comm.nranks; ++r)
        for (size_t t = 0; t < gotp[r].size(); t += 2) {
            el[pos[gotp[r][t] - lo]++] = (int)gotp[r][t + 1];
            need.push_back(gotp[r][t + 1]);
        }
    erp.upload(ec.data(), ec.size());
    ecol.upload(el.data(), el.size());
    return build_halo_plan(comm, L.A.col_starts, std::move(need));
}

// the C/F states cf.  The S^T adjacency, the keys, the off-rank lists and their halo are the
// stage's own: freed on return, before interpolation (the level's peak)
void pmis_split(LevelCtx& L, const DCsr& Sv, DevBuf<int>& cf) {
    hipStream_t s = L.s;
    const HostComm& comm = L.comm;
    const int n = L.n, lo = L.lo;
    const bool dist = L.dist;
    // |S^T_i| and the S^T adjacency of the local-local part
    DevBuf<int> tcnt, trp, tcol, cursor;
    tcnt.alloc((size_t)n + 1);
    HIP_CHECK(hipMemsetAsync(tcnt.p, 0, sizeof(int) * tcnt.n, s));
    launch_rows(s, n, col_count_kernel, Sv, tcnt.p);
    trp.alloc((size_t)n + 1);
    const int64_t tnnz = exclusive_scan(s, tcnt.p, trp.p, n, L.tmp);
    tcol.alloc((size_t)std::max<int64_t>(tnnz, 1));
    cursor.alloc((size_t)n + 1);
    HIP_CHECK(hipMemcpyAsync(cursor.p, trp.p, sizeof(int) * (n + 1), hipMemcpyDeviceToDevice, s));
    launch_rows(s, n, transpose_fill_kernel, Sv, cursor.p, tcol.p);
    DevBuf<int> erp, ecol;
    DevHalo H;
    H.build(dist ? offrank_dependents(L, Sv, erp, ecol) : HaloPlan());
    const Dist Dn = H.dist(lo, n);
    DevBuf<unsigned long long> key, hkey, nu;
    DevBuf<int> hcf;
    DevBuf<unsigned char> newc;
    key.alloc((size_t)std::max(n, 1));
    cf.alloc((size_t)std::max(n, 1));
    newc.alloc((size_t)std::max(n, 1));
    nu.alloc(1);
    hkey.alloc(1);
    hcf.alloc(1);
    launch_rows(s, n, pmis_init_kernel, n, lo, tcnt.p, dist ? erp.p : nullptr, (unsigned long long)L.seed(), key.p,
                cf.p);
    if (dist) H.forward(s, comm, key.p, hkey);
    for (int round = 0;; ++round) {
        AMG_CHECK(round <= L.A.n_global_rows, "PMIS did not terminate");
        if (dist) H.forward(s, comm, cf.p, hcf);
        launch_rows(s, n, pmis_select_kernel, Sv, Dn, trp.p, tcol.p, dist ? erp.p : nullptr,
                    dist ? ecol.p : nullptr, key.p, hkey.p, cf.p, hcf.p, newc.p);
        launch_rows(s, n, pmis_apply_kernel, n, newc.p, cf.p);
        if (dist) H.forward(s, comm, cf.p, hcf);
        HIP_CHECK(hipMemsetAsync(nu.p, 0, sizeof(unsigned long long), s));
        launch_rows(s, n, pmis_fpass_kernel, Sv, Dn, cf.p, hcf.p, nu.p);
        const int64_t left = (int64_t)read_scalar(s, nu.p);
        if ((dist ? comm.allreduce_sum(left) : left) == 0) break;
    }
}

// the multicolour ordering of A's rows: pmis_split's stages on the operator's own
// pattern -- the local transpose adjacency, the off-rank dependents and their halo, synchronous
// rounds with one scalar back per round.  Collective on a distributed level
void colour_rows(LevelCtx& L, Colouring& out) {
    hipStream_t s = L.s;
    const HostComm& comm = L.comm;
    const int n = L.n, lo = L.lo;
    const bool dist = L.dist;
    const DCsr& Av = L.Av;
    DevBuf<int> tcnt, trp, tcol, cursor;
    tcnt.alloc((size_t)n + 1);
    HIP_CHECK(hipMemsetAsync(tcnt.p, 0, sizeof(int) * tcnt.n, s));
    launch_rows(s, n, col_count_kernel, Av, tcnt.p);
    trp.alloc((size_t)n + 1);
    const int64_t tnnz = exclusive_scan(s, tcnt.p, trp.p, n, L.tmp);
    tcol.alloc((size_t)std::max<int64_t>(tnnz, 1));
    cursor.alloc((size_t)n + 1);
    HIP_CHECK(hipMemcpyAsync(cursor.p, trp.p, sizeof(int) * (n + 1), hipMemcpyDeviceToDevice, s));
    launch_rows(s, n, transpose_fill_kernel, Av, cursor.p, tcol.p);
    DevBuf<int> erp, ecol;
    DevHalo H;
    H.build(dist ? offrank_dependents(L, Av, erp, ecol) : HaloPlan());
    const Dist Dn = H.dist(lo, n);
    DevBuf<unsigned> key, hkey;
    DevBuf<int> colour, hcolour, newc, cmax;
    DevBuf<unsigned long long> left;
    key.alloc((size_t)std::max(n, 1));
    colour.alloc((size_t)std::max(n, 1));
    newc.alloc((size_t)std::max(n, 1));
    hkey.alloc(1);
    hcolour.alloc(1);
    left.alloc(1);
    cmax.alloc(1);
    HIP_CHECK(hipMemsetAsync(cmax.p, 0xFF, sizeof(int), s));  // -1: no colour yet
    launch_rows(s, n, colour_init_kernel, n, lo, (unsigned long long)L.seed(), key.p, colour.p);
    if (dist) H.forward(s, comm, key.p, hkey);
    int64_t rows_left = dist ? comm.allreduce_sum(n) : n;
    int round = 0;
    for (; rows_left > 0; ++round) {
        AMG_CHECK(round <= L.A.n_global_rows, "multicolour ordering did not terminate");
        if (dist) H.forward(s, comm, colour.p, hcolour);
        launch_rows(s, n, colour_select_kernel, Av, Dn, trp.p, tcol.p, dist ? erp.p : nullptr,
                    dist ? ecol.p : nullptr, key.p, hkey.p, colour.p, hcolour.p, newc.p);
        HIP_CHECK(hipMemsetAsync(left.p, 0, sizeof(unsigned long long), s));
        launch_rows(s, n, colour_apply_kernel, n, newc.p, colour.p, left.p, cmax.p);
        const int64_t l = (int64_t)read_scalar(s, left.p);
        rows_left = dist ? comm.allreduce_sum(l) : l;
    }
    int64_t nc = (int64_t)read_scalar(s, cmax.p) + 1;
    if (dist)
        for (int64_t v : comm.allgather(nc)) nc = std::max(nc, v);
    out.colour = download_ints(s, colour.p, n);
    out.n_colours = (int32_t)nc;
    out.rounds = round;
}

// coarse numbering: C points in row order, ranks in order
struct CoarseIds : Pinned {
    std::vector<int64_t> cstarts;  // the coarse partition
    std::vector<int> host;         // coarse id of a local C row, else -1
    DevBuf<int> cmap;              // the same on the device
};

void coarse_numbering(LevelCtx& L, const DevBuf<int>& cf, std::vector<int32_t>& split, CoarseIds& C) {
    const HostComm& comm = L.comm;
    const int n = L.n;
    split = download_ints(L.s, cf.p, n);
    int64_t ncl = 0;
    for (int32_t v : split) ncl += v == ST_C;
    C.cstarts.assign(comm.nranks + 1, 0);
    {
        const std::vector<int64_t> counts = comm.allgather(ncl);
        for (int r = 0; r < comm.nranks; ++r) C.cstarts[r + 1] = C.cstarts[r] + counts[r];
    }
    AMG_CHECK(C.cstarts[comm.nranks] < INT_MAX, "device setup: coarse level exceeds int32 indexing");
    C.host.assign((size_t)std::max(n, 1), -1);
    for (int i = 0, c = (int)C.cstarts[comm.rank]; i < n; ++i)
        if (split[i] == ST_C) C.host[i] = c++;
    C.cmap.upload(C.host.data(), C.host.size());
}

// A's halo: states and coarse ids of the off-rank columns, and their ghost rows
struct AHalo : Pinned {
    DevHalo AH;
    GhostRows G;
    DevBuf<int> acf, acmap, grp, gcol;
    DevBuf<double> gval;
    ARows rows(const LevelCtx& L) const { return ARows{L.Av, AH.dist(L.lo, L.n), grp.p, gcol.p, gval.p}; }
};

void a_halo_and_ghost_rows(LevelCtx& L, const std::vector<int32_t>& split, const CoarseIds& C, AHalo& H) {
    const HostComm& comm = L.comm;
    H.AH.build(L.dist ? halo_plan_for_cols(comm, L.A) : HaloPlan());
    const HaloPlan& aplan = H.AH.plan;
    H.acf.alloc(1);
    H.acmap.alloc(1);
    if (!L.dist) {
        H.grp.alloc(1);
        H.gcol.alloc(1);
        H.gval.alloc(1);
        return;
    }
    GhostRows& G = H.G;
    G = fetch_rows(comm, aplan, L.A);
    std::vector<int32_t> hcfa(aplan.n_halo());
    std::vector<int64_t> cm64(C.host.begin(), C.host.begin() + L.n), hcm64(aplan.n_halo());
    aplan.forward(comm, split.data(), hcfa.data());
    aplan.forward(comm, cm64.data(), hcm64.data());
    std::vector<int> hcma(hcm64.begin(), hcm64.end());
    H.acf.upload(hcfa.data(), hcfa.size());
    H.acmap.upload(hcma.data(), hcma.size());
    AMG_CHECK(G.rp.back() < INT_MAX, "device setup: ghost rows exceed int32 indexing");
    std::vector<int> gr(G.rp.begin(), G.rp.end()), gc(G.col.begin(), G.col.end());
    H.grp.upload(gr.data(), gr.size());
    H.gcol.upload(gc.data(), std::max<size_t>(gc.size(), 1));
    H.gval.upload(G.val.data(), std::max<size_t>(G.val.size(), 1));
}

// P's rows: classical interpolation a thread or a wave per row, or extended+i (X: the state halo
// two deep, then count / scan / fill too)
void interpolate(LevelCtx& L, const DCsr& Sv, const DevBuf<int>& cf, const CoarseIds& C, const AHalo& H, ExtInterp& X,
                 DevRows<int>& p) {
    hipStream_t s = L.s;
    const int n = L.n;
    const ARows Ar = H.rows(L);
    const bool ext = L.opt.interp == AMG_INTERP_EXT_I;
    if (ext)
        X.init(s, L.comm, L.A, H.AH.plan, H.G, Ar, Sv, cf.p, C.cmap.p, (int)C.cstarts[L.comm.nranks], L.opt);
    // long rows (the Galerkin levels): a wave per row (interp_wave_kernel); AMG_INTERP_WAVE_NPR
    // sets the average row length from which it is taken (default 12; 0: always)
    const char* wenv = std::getenv("AMG_INTERP_WAVE_NPR");
    const int wave_npr = wenv && *wenv ? std::atoi(wenv) : 12;
    const bool wave = n > 0 && L.A.nnz() >= (int64_t)wave_npr * n;
    const dim3 wgrid((unsigned)((n + kIwWaves - 1) / kIwWaves)), wblk(64 * kIwWaves);
    build_rows_with(
        L, p,
        [&](int* cnt) {
            if (n && ext)
                X.count(cnt);
            else if (wave)
                hipLaunchKernelGGL(interp_wave_kernel<false>, wgrid, wblk, 0, s, Ar, Sv, cf.p, H.acf.p, C.cmap.p,
                                   H.acmap.p, cnt, nullptr, nullptr, nullptr);
            else
                launch_rows(s, n, interp_kernel<false>, Ar, Sv, cf.p, H.acf.p, C.cmap.p, H.acmap.p, cnt, nullptr,
                            nullptr, nullptr);
        },
        [&](const int* prp, int* pcol, double* pval) {
            if (n && ext)
                X.fill(prp, pcol, pval);
            else if (wave)
                hipLaunchKernelGGL(interp_wave_kernel<true>, wgrid, wblk, 0, s, Ar, Sv, cf.p, H.acf.p, C.cmap.p,
                                   H.acmap.p, nullptr, prp, pcol, pval);
            else
                launch_rows(s, n, interp_kernel<true>, Ar, Sv, cf.p, H.acf.p, C.cmap.p, H.acmap.p, nullptr, prp, pcol,
                            pval);
        });
}

template <class I, class V>
void download_index(hipStream_t s, const I* p, int64_t n, V& out) {
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 columns");
    if constexpr (std::is_same<I, int>::value) {
        const std::vector<int32_t> h = download_ints(s, p, n);
        out.assign(h.begin(), h.end());
    } else {
        out.resize((size_t)n);
        copy_to_host(out.data(), p, sizeof(long long) * n, s);
    }
}

// P on the host, columns partitioned by cstarts; with imgs, the device arrays become P's image
// (where it was computed, for the transpose and the Galerkin product) -- int32 or int64 indices
template <class I>
void take_P(LevelCtx& L, DevRows<I>& p, const std::vector<int64_t>& cstarts, HostCSR& P, SetupImages* imgs) {
    P = HostCSR();
    P.n_global_rows = L.A.n_global_rows;
    P.n_global_cols = cstarts[L.comm.nranks];
    P.row_starts = L.A.row_starts;
    P.col_starts = cstarts;
    download_index(L.s, p.rp.p, (int64_t)L.n + 1, P.rp);
    download_index(L.s, p.col.p, p.nnz, P.col);
    P.val.resize((size_t)p.nnz);
    copy_to_host(P.val.data(), p.val.p, sizeof(double) * p.nnz, L.s);
    if (!imgs) return;
    std::unique_ptr<DevCsr> d(new DevCsr());
    if constexpr (std::is_same<I, int>::value) {
        d->rp32 = std::move(p.rp);
        d->col32 = std::move(p.col);
    } else {
        d->rp64 = std::move(p.rp);
        d->col64 = std::move(p.col);
    }
    d->val = std::move(p.val);
    imgs->put(P, std::move(d));
}

// PMIS coarsening with classical or extended+i interpolation (host_setup.cpp pmis_split /
// interp_classical / interp_ext_i)
bool pmis_level(LevelCtx& L, HostCSR& P, std::vector<int32_t>& split, SetupImages& im, int64_t* ext_stats) {
    DevS S;
    classical_strength(L, S);
    L.tm.lap("  device strength");
    DevBuf<int> cf;
    pmis_split(L, view(L, S), cf);
    L.tm.lap("  device PMIS");
    CoarseIds C;
    coarse_numbering(L, cf, split, C);
    AHalo H;
    a_halo_and_ghost_rows(L, split, C, H);
    L.tm.lap("  device coarse ids + ghost rows");
    const bool ext = L.opt.interp == AMG_INTERP_EXT_I;
    ExtInterp X;
    DevRows<int> p;
    interpolate(L, view(L, S), cf, C, H, X, p);
    take_P(L, p, C.cstarts, P, &im);
    if (ext && ext_stats) ext_stats[0] = (int64_t)X.slots.size(), ext_stats[1] = X.launches;
    L.tm.lap(ext ? "  device interpolation (" + std::to_string(X.slots.size()) + " scratch rows)"
                 : std::string("  device interpolation"));
    return true;
}

// ---- SA level: the stages of sa_level ---------------------------------------------------------
// A's halo: a_jj of other ranks' columns, then the MIS(2) tuples, aggregate ids and weights of the
// strong neighbours (S is a subset of A's pattern); read by every stage
struct SaHalo : Pinned {
    double theta = 0.0;
    DevHalo AH;
    DevBuf<double> d, hd;  // a_ii, and of the halo columns
};

void symmetric_strength(LevelCtx& L, SaHalo& H, DevS& S) {
    hipStream_t s = L.s;
    const int n = L.n;
    H.theta = sa_theta(L.opt.strong_threshold, L.level);
    H.AH.build(L.dist ? halo_plan_for_cols(L.comm, L.A) : HaloPlan());
    const Dist Da = H.AH.dist(L.lo, n);
    H.d.alloc((size_t)std::max(n, 1));
    H.hd.alloc(1);
    launch_rows(s, n, diagonal_kernel, L.Av, H.d.p);
    if (L.dist) H.AH.forward(s, L.comm, H.d.p, H.hd);
    build_rows(L, S, strength_symmetric_kernel<false>, strength_symmetric_kernel<true>, L.Av, Da, H.d.p, H.hd.p,
               H.theta);
}

// the MIS(2) rounds: st[i] == M_IN marks the roots.  The hops swap the raw pointers of h0 / h1
// and l0 / l1, which are all this function's
void mis2_rounds(LevelCtx& L, const SaHalo& H, const DCsr& Sv, DevBuf<int>& st) {
    hipStream_t s = L.s;
    const HostComm& comm = L.comm;
    const int n = L.n, lo = L.lo;
    const bool dist = L.dist;
    const Dist Da = H.AH.dist(lo, n);
    const size_t nn = (size_t)std::max(n, 1);
    std::vector<unsigned> hs(nn);
    for (int i = 0; i < n; ++i) hs[i] = hash32(lo + i, L.seed());
    DevBuf<unsigned> dhs;
    dhs.upload(hs.data(), hs.size());
    DevBuf<unsigned long long> h0, l0, h1, l1, hh, hl, nu;
    h0.alloc(nn), l0.alloc(nn), h1.alloc(nn), l1.alloc(nn), nu.alloc(1), hh.alloc(1), hl.alloc(1);
    {
        std::vector<int> init(nn, M_U);
        st.upload(init.data(), init.size());
    }
    for (int round = 0;; ++round) {
        AMG_CHECK(round <= L.A.n_global_rows, "MIS(2) did not terminate");
        launch_rows(s, n, mis2_tuple_kernel, n, lo, st.p, dhs.p, h0.p, l0.p);
        for (int hop = 0; hop < 2; ++hop) {
            if (dist) {
                H.AH.forward(s, comm, h0.p, hh);
                H.AH.forward(s, comm, l0.p, hl);
            }
            launch_rows(s, n, mis2_hop_kernel, Sv, Da, h0.p, l0.p, hh.p, hl.p, h1.p, l1.p);
            std::swap(h0.p, h1.p);
            std::swap(l0.p, l1.p);
        }
        HIP_CHECK(hipMemsetAsync(nu.p, 0, sizeof(unsigned long long), s));
        launch_rows(s, n, mis2_update_kernel, n, lo, h0.p, l0.p, st.p, nu.p);
        const int64_t left = (int64_t)read_scalar(s, nu.p);
        if ((dist ? comm.allreduce_sum(left) : left) == 0) break;
    }
}

struct Aggregates : Pinned {
    std::vector<int64_t> astarts;  // the partition of the aggregates (the coarse columns)
    DevBuf<int> agg;               // aggregate of every local row (split on the host)
};

// roots numbered in global row order (ranks in order) by an exclusive scan of the root flags;
// aggr = a root's aggregate id, -1; then the two joining passes
void mis2_aggregate(LevelCtx& L, const SaHalo& H, const DCsr& Sv, Aggregates& ag, std::vector<int32_t>& split) {
    hipStream_t s = L.s;
    const HostComm& comm = L.comm;
    const int n = L.n;
    const bool dist = L.dist;
    const Dist Da = H.AH.dist(L.lo, n);
    const size_t nn = (size_t)std::max(n, 1);
    DevBuf<int> st;
    mis2_rounds(L, H, Sv, st);
    DevBuf<int> rflag, rpos;
    rflag.alloc(nn + 1);
    rpos.alloc(nn + 1);
    HIP_CHECK(hipMemsetAsync(rflag.p, 0, sizeof(int) * rflag.n, s));
    launch_rows(s, n, root_flag_kernel, n, st.p, rflag.p);
    const int64_t nroot = exclusive_scan(s, rflag.p, rpos.p, n, L.tmp);
    ag.astarts.assign(comm.nranks + 1, 0);
    {
        const std::vector<int64_t> counts = comm.allgather(nroot);
        for (int r = 0; r < comm.nranks; ++r) ag.astarts[r + 1] = ag.astarts[r] + counts[r];
    }
    AMG_CHECK(ag.astarts[comm.nranks] < INT_MAX, "device setup: coarse level exceeds int32 indexing");
    DevBuf<int> aggr, haggr, a1, ha1;
    DevBuf<unsigned long long> nu;
    aggr.alloc(nn);
    launch_rows(s, n, root_id_kernel, n, st.p, rpos.p, (int)ag.astarts[comm.rank], aggr.p);
    haggr.alloc(1);
    ha1.alloc(1);
    a1.alloc(nn);
    ag.agg.alloc(nn);
    nu.alloc(1);
    if (dist) H.AH.forward(s, comm, aggr.p, haggr);
    launch_rows(s, n, mis2_pass1_kernel, Sv, Da, aggr.p, haggr.p, a1.p);
    if (dist) H.AH.forward(s, comm, a1.p, ha1);
    HIP_CHECK(hipMemsetAsync(nu.p, 0, sizeof(unsigned long long), s));
    launch_rows(s, n, mis2_pass2_kernel, Sv, Da, a1.p, ha1.p, ag.agg.p, nu.p);
    if (read_scalar(s, nu.p)) throw Error(AMG_ERR_INTERNAL, "MIS(2): unaggregated node");
    split = download_ints(s, ag.agg.p, n);
}

// aggregate sizes (owners count their members, members elsewhere report in), T = 1 /
// sqrt(|aggregate|): dt, and hdt of the halo columns (A_F T)
struct Tentative : Pinned {
    DevBuf<double> dt, hdt;
};

void tentative_weights(LevelCtx& L, const SaHalo& H, const std::vector<int32_t>& split,
                       const std::vector<int64_t>& astarts, Tentative& T) {
    const HostComm& comm = L.comm;
    const int n = L.n;
    const bool dist = L.dist;
    const int64_t alo = astarts[comm.rank], ahi = astarts[comm.rank + 1];
    std::vector<int64_t> size((size_t)(ahi - alo), 0);
    std::vector<std::vector<int64_t>> sendc(comm.nranks);
    std::vector<int64_t> needa;
    if (!dist) {  // every aggregate is this rank's: counted in parallel (integer counts)
#pragma omp parallel for schedule(static)
        for (int i = 0; i < n; ++i) {
#pragma omp atomic
            size[split[i] - alo]++;
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const int64_t a = split[i];
            if (a >= alo && a < ahi) {
                size[a - alo]++;
            } else {
                sendc[owner_of(astarts, a)].push_back(a);
                needa.push_back(a);
            }
        }
    }
    if (dist) {
        const auto got = comm.exchange(sendc);
        for (int r = 0; r < comm.nranks; ++r)
            for (int64_t a : got[r]) size[a - alo]++;
    }
    HaloPlan splan;
    std::vector<int64_t> hsize;
    if (dist) {
        splan = build_halo_plan(comm, astarts, std::move(needa));
        hsize.resize(splan.n_halo());
        splan.forward(comm, size.data(), hsize.data());
    }
    std::vector<double> tv((size_t)std::max(n, 1));
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        const int64_t a = split[i];
        const int64_t sz = (a >= alo && a < ahi) ? size[a - alo] : hsize[splan.find(a)];
        tv[i] = 1.0 / std::sqrt((double)sz);
    }
    T.dt.upload(tv.data(), tv.size());
    T.hdt.alloc(1);
    if (dist) H.AH.forward(L.s, comm, T.dt.p, T.hdt);
}

// the filtered operator A_F (r6): the diagonal + the strong couplings, weak ones lumped; returns
// rho(D^-1 A_F)
double filtered_operator_and_rho(LevelCtx& L, const SaHalo& H, DevS& F) {
    hipStream_t s = L.s;
    const int n = L.n;
    const Dist Da = H.AH.dist(L.lo, n);
    build_rows(L, F, sa_filter_kernel<false>, sa_filter_kernel<true>, L.Av, Da, H.d.p, H.hd.p, H.theta);
    const DCsr Fv = view(L, F);
    DevBuf<double> x, y, hx;
    x.alloc((size_t)std::max(n, 1));
    y.alloc((size_t)std::max(n, 1));
    hx.alloc(1);
    return power_iteration(s, L.comm, L.dist, n, L.lo, L.seed(), kSaRhoIters, x.p, y.p, [&](unsigned long long* mx) {
        if (L.dist) H.AH.forward(s, L.comm, x.p, hx);
        launch_rows(s, n, sa_power_kernel, Fv, Da, x.p, hx.p, H.d.p, y.p, mx);
    });
}

// P = T - (omega / a_ii) A_F T on the device, on any number of ranks
void smooth_P(LevelCtx& L, const SaHalo& H, const Aggregates& ag, const Tentative& T, const DevS& F, double omega,
              DevRows<long long>& p) {
    hipStream_t s = L.s;
    const int n = L.n;
    const Dist Da = H.AH.dist(L.lo, n);
    const DCsr Fv = view(L, F);
    DevBuf<int> hagg, skey;
    DevBuf<double> sval;
    hagg.alloc(1);
    if (L.dist) H.AH.forward(s, L.comm, ag.agg.p, hagg);
    skey.alloc((size_t)std::max<int64_t>(F.nnz, 1));
    sval.alloc((size_t)std::max<int64_t>(F.nnz, 1));
    build_rows(L, p, sa_smooth_kernel<false>, sa_smooth_kernel<true>, Fv, Da, ag.agg.p, hagg.p, T.dt.p, T.hdt.p,
               H.d.p, omega, skey.p, sval.p);
}

// smoothed aggregation (host_setup.cpp strength_symmetric, mis2_aggregate, sa_prolongator)
bool sa_level(LevelCtx& L, HostCSR& P, std::vector<int32_t>& split, SetupImages& im) {
    SaHalo H;
    Aggregates ag;
    {
        DevS S;  // the strength graph: the aggregation's alone
        symmetric_strength(L, H, S);
        L.tm.lap("  device strength");
        mis2_aggregate(L, H, view(L, S), ag, split);
        L.tm.lap("  device aggregation");
    }
    Tentative T;
    tentative_weights(L, H, split, ag.astarts, T);
    L.tm.lap("  device tentative prolongator");
    DevS F;
    const double rho = filtered_operator_and_rho(L, H, F);
    const double omega = rho > 0.0 ? (4.0 / 3.0) / rho : 0.0;
    L.tm.lap("  device filtered operator + rho");
    DevRows<long long> p;
    smooth_P(L, H, ag, T, F, omega, p);
    // one rank keeps P as the setup's image (N ranks: the transpose and SpGEMM build their own)
    take_P(L, p, ag.astarts, P, L.dist ? nullptr : &im);
    L.tm.lap("  device smoothed prolongator");
    return true;
}

}  // namespace

double power_iteration(hipStream_t s, const HostComm& comm, bool dist, int n, int64_t first_gid, uint64_t seed,
                       int iters, double* x, const double* y, const std::function<void(unsigned long long* m)>& step) {
    DevBuf<unsigned long long> mx;
    mx.alloc(1);
    auto global_max = [&]() {
        const unsigned long long bits = read_scalar(s, mx.p);
        double m;
        std::memcpy(&m, &bits, sizeof(m));
        return dist ? comm.allreduce_max(m) : m;
    };
    launch_uniform(s, n, first_gid, seed, x);
    HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(unsigned long long), s));
    launch_rows(s, n, max_abs_kernel, n, x, mx.p);
    const double m0 = global_max();
    if (m0 > 0.0) launch_rows(s, n, div_scalar_kernel, n, x, m0, x);
    double lam = 0.0;
    for (int it = 0; it < iters; ++it) {
        HIP_CHECK(hipMemsetAsync(mx.p, 0, sizeof(unsigned long long), s));
        step(mx.p);
        HIP_CHECK(hipGetLastError());
        lam = global_max();
        if (lam == 0.0) break;
        launch_rows(s, n, div_scalar_kernel, n, y, lam, x);
    }
    return lam;
}

// One level of the setup on the device: P and the integer split (C/F marker for RS-family
// coarsening, aggregate id for SA), on any number of ranks.  Each rank works on its rows
// with global column ids; the states of other ranks' points arrive through halo forwards
// (pack on the device, the setup exchange on the host) -- exactly the synchronous rounds of
// host_setup.cpp pmis_split / interp_classical / interp_ext_i / mis2_aggregate / sa_prolongator, so the
// hierarchy is bit-identical to the host path's at every rank count.  Returns false for
// Ruge-Stueben (the serial first pass stays on the host).
bool level_setup_device(Context& ctx, const HostComm& comm, const HostCSR& A, const amg_options& opt,
                        int level, HostCSR& P, std::vector<int32_t>& split, SetupImages* imgs, int64_t* ext_stats) {
    if (ext_stats) ext_stats[0] = ext_stats[1] = 0;
    // Ruge-Stueben (serial first pass): the host path
    if (opt.coarsen == AMG_COARSEN_RS) return false;
    if (comm.nranks == 1 && A.nrows() == 0) return false;
    LevelCtx L(ctx.stream, comm, A, opt, level);
    // A on the device: the setup's image (uploaded once, or left there by the previous level's
    // Galerkin product); a caller without images gets this level's own
    SetupImages local;
    SetupImages& im = imgs ? *imgs : local;
    DevCsr& DA = im.get(A);
    AMG_CHECK(A.nrows() < INT_MAX && A.n_global_cols < INT_MAX, "device setup: level exceeds int32 indexing");
    DA.ensure_rp32(L.s);
    DA.ensure_col32(L.s);
    L.Av = DCsr{DA.rp32.p, DA.col32.p, DA.val.p, L.n, L.lo};
    if (opt.coarsen == AMG_COARSEN_PMIS) return pmis_level(L, P, split, im, ext_stats);
    AMG_CHECK(opt.coarsen == AMG_COARSEN_SA, "unknown coarsening");
    return sa_level(L, P, split, im);
}

// The multicolour ordering of A's rows with the hash keys of `seed` (a solver's level l:
// opt.seed + l).  imgs: A's device image where a setup holds it; otherwise A is uploaded for
// the call.  Collective over the ranks of comm.
Colouring colour_device(Context& ctx, const HostComm& comm, const HostCSR& A, uint64_t seed, SetupImages* imgs) {
    Colouring out;
    AMG_CHECK(A.n_global_rows == A.n_global_cols && A.row_starts == A.col_starts,
              "multicolour ordering needs a square matrix");
    if (comm.nranks == 1 && A.nrows() == 0) return out;
    AMG_CHECK(A.nrows() < INT_MAX && A.n_global_cols < INT_MAX, "multicolour ordering: level exceeds int32 indexing");
    amg_options opt{};
    opt.seed = seed;
    LevelCtx L(ctx.stream, comm, A, opt, 0);
    SetupImages local;
    SetupImages& im = imgs && imgs->find(A) ? *imgs : local;
    DevCsr& DA = im.get(A);
    DA.ensure_rp32(L.s);
    DA.ensure_col32(L.s);
    L.Av = DCsr{DA.rp32.p, DA.col32.p, DA.val.p, L.n, L.lo};
    colour_rows(L, out);
    return out;
}

namespace {

void sort_pairs_stable(hipStream_t s, const int* keys_in, int* keys_out, const int* vals_in, int* vals_out, int m,
                       int64_t key_range, DevBuf<char>& tmp) {
    int bits = 1;
    while (bits < 31 && (1ll << bits) < key_range) ++bits;
    size_t bytes = 0;
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, m, 0, bits, s));
    if (tmp.n < bytes) tmp.alloc(bytes);
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, keys_in, keys_out, vals_in, vals_out, m, 0, bits, s));
}

// R = P^T on N ranks (host_comm.cpp transpose(), the same records and exchange): each rank
// sorts its entries by global column on the device (stable: fine rows stay ascending), ships
// each owner its contiguous record range (one all-to-all-v), and the owner sorts what it
// received by local row, stably -- rank order, then ascending fine row, as the host
// transpose places them.  Bit-identical to it.
bool transpose_device_dist(Context& ctx, const HostComm& comm, const HostCSR& P, HostCSR& R, SetupImages* imgs) {
    hipStream_t s = ctx.stream;
    const int64_t n = P.nrows(), nnz = P.nnz(), nc = P.n_global_cols;
    const int64_t lo = P.col_starts[comm.rank], m_rows = P.col_starts[comm.rank + 1] - lo;
    // every rank takes the same path (the exchange is collective)
    int64_t ok = n < INT_MAX && nnz < INT_MAX && nc < INT_MAX;
    for (int64_t v : comm.allgather(ok)) ok = ok && v;
    if (!ok) return false;
    static_assert(sizeof(TRec) == 24, "record layout");
    DevBuf<char> tmp;
    const int nr = comm.nranks, me = comm.rank;
    // records sorted by column: owner o's range [off[o], off[o + 1]); this rank's own range
    // stays on the device, only the others' travel through the host exchange
    std::vector<long long> off((size_t)nr + 1, 0);
    DevBuf<TRec> recs;
    std::vector<TRec> sbuf;
    if (nnz) {
        SetupImages local;
        DevCsr& dP = (imgs ? *imgs : local).get(P);
        dP.ensure_rp32(s);
        dP.ensure_col32(s);
        DevBuf<int> keys_out, idx_in, idx_out, rowof;
        DevBuf<long long> dbound, doff;
        keys_out.alloc(nnz);
        idx_in.alloc(nnz);
        idx_out.alloc(nnz);
        rowof.alloc(nnz);
        recs.alloc(nnz);
        launch_rows(s, nnz, iota_kernel, (int)nnz, idx_in.p);
        launch_rows(s, n, expand_rows_kernel, dP.rp32.p, (int)n, rowof.p);
        sort_pairs_stable(s, dP.col32.p, keys_out.p, idx_in.p, idx_out.p, (int)nnz, nc, tmp);
        launch_rows(s, nnz, transpose_records_kernel, (int)nnz, keys_out.p, idx_out.p, rowof.p, dP.val.p,
                    (long long)P.row_starts[me], recs.p);
        std::vector<long long> bound(P.col_starts.begin() + 1, P.col_starts.end());
        dbound.upload(bound.data(), bound.size());
        doff.alloc((size_t)nr);
        launch_rows(s, nr, owner_bounds_kernel, (int)nnz, keys_out.p, nr, dbound.p, doff.p);
        HIP_CHECK(hipGetLastError());
        copy_to_host(off.data() + 1, doff.p, sizeof(long long) * nr, s);
        off[nr] = nnz;
        const int64_t nsend = nnz - (off[me + 1] - off[me]);
        sbuf.resize((size_t)nsend);
        copy_to_host(sbuf.data(), recs.p, sizeof(TRec) * off[me], nullptr);
        copy_to_host(sbuf.data() + off[me], recs.p + off[me + 1], sizeof(TRec) * (nnz - off[me + 1]), nullptr);
    }
    std::vector<int64_t> cnt(nr, 0), sb(nr), rb(nr);
    for (int o = 0; o < nr; ++o) cnt[o] = off[o + 1] - off[o];
    const std::vector<int64_t> rcnt = comm.alltoall_counts(cnt);
    int64_t rtot = 0, rfor = 0, before = 0;
    for (int o = 0; o < nr; ++o) {
        sb[o] = o == me ? 0 : cnt[o] * (int64_t)sizeof(TRec);
        rb[o] = o == me ? 0 : rcnt[o] * (int64_t)sizeof(TRec);
        rtot += rcnt[o];
        if (o != me) rfor += rcnt[o];
        if (o < me) before += rcnt[o];
    }
    std::vector<TRec> rbuf((size_t)rfor);
    comm.alltoallv(sbuf.data(), sb, rbuf.data(), rb);
    std::vector<TRec>().swap(sbuf);
    AMG_CHECK(rtot < INT_MAX && m_rows < INT_MAX, "device transpose: rows exceed int32 indexing");
    R = HostCSR();
    R.n_global_rows = nc;
    R.n_global_cols = P.n_global_rows;
    R.row_starts = P.col_starts;
    R.col_starts = P.row_starts;
    R.rp.assign((size_t)m_rows + 1, 0);
    R.col.resize((size_t)rtot);
    R.val.resize((size_t)rtot);
    if (rtot) {
        // received records in rank order: [ranks < me | own range (device to device) | ranks > me]
        DevBuf<TRec> drec;
        DevBuf<int> key, key_out, idx_in, idx_out, cntd, rrp;
        DevBuf<long long> rcol;
        DevBuf<double> rval;
        const int64_t own = rtot - rfor;
        drec.alloc((size_t)rtot);
        if (before) copy_to_device(drec.p, rbuf.data(), sizeof(TRec) * before);
        if (own)
            HIP_CHECK(hipMemcpyAsync(drec.p + before, recs.p + off[me], sizeof(TRec) * own, hipMemcpyDeviceToDevice, s));
        if (rfor > before)
            copy_to_device(drec.p + before + own, rbuf.data() + before, sizeof(TRec) * (rfor - before));
        std::vector<TRec>().swap(rbuf);
        HIP_CHECK(hipStreamSynchronize(s));
        recs.reset();
        key.alloc(rtot);
        key_out.alloc(rtot);
        idx_in.alloc(rtot);
        idx_out.alloc(rtot);
        launch_rows(s, rtot, record_rows_kernel, (int)rtot, drec.p, (long long)lo, key.p);
        launch_rows(s, rtot, iota_kernel, (int)rtot, idx_in.p);
        sort_pairs_stable(s, key.p, key_out.p, idx_in.p, idx_out.p, (int)rtot, m_rows, tmp);
        rcol.alloc(rtot);
        rval.alloc(rtot);
        launch_rows(s, rtot, gather_records_kernel, (int)rtot, idx_out.p, drec.p, rcol.p, rval.p);
        cntd.alloc((size_t)m_rows + 1);
        HIP_CHECK(hipMemsetAsync(cntd.p, 0, sizeof(int) * cntd.n, s));
        launch_rows(s, rtot, count_cols_kernel, (int)rtot, key.p, cntd.p);
        rrp.alloc((size_t)m_rows + 1);
        exclusive_scan(s, cntd.p, rrp.p, (int)m_rows, tmp);
        HIP_CHECK(hipGetLastError());
        const std::vector<int> hrp = download_ints(s, rrp.p, m_rows + 1);
        R.rp.assign(hrp.begin(), hrp.end());
        copy_to_host(R.col.data(), rcol.p, sizeof(long long) * rtot, s);
        copy_to_host(R.val.data(), rval.p, sizeof(double) * rtot, nullptr);
        if (imgs) {  // R where it was computed, for the Galerkin product
            std::unique_ptr<DevCsr> d(new DevCsr());
            d->rp32 = std::move(rrp);
            d->col64 = std::move(rcol);
            d->val = std::move(rval);
            imgs->put(R, std::move(d));
        }
    }
    return true;
}

}  // namespace

// R = P^T on the device for one rank: stable radix sort of the entries by column keeps each
// R row in ascending fine-row order, like transpose().
bool transpose_device(Context& ctx, const HostComm& comm, const HostCSR& P, HostCSR& R, SetupImages* imgs) {
    if (comm.nranks != 1) return transpose_device_dist(ctx, comm, P, R, imgs);
    hipStream_t s = ctx.stream;
    const int64_t n = P.nrows(), nnz = P.nnz(), nc = P.n_global_cols;
    if (nnz == 0 || n >= INT_MAX || nnz >= INT_MAX || nc >= INT_MAX) return false;
    DevBuf<int> keys_out, idx_in, idx_out, rowof, cnt, rrp;
    DevBuf<long long> rcol;
    DevBuf<double> rval;
    DevBuf<char> tmp;
    SetupImages local;
    DevCsr& dP = (imgs ? *imgs : local).get(P);  // P's image (left on the device by the level setup)
    dP.ensure_rp32(s);
    dP.ensure_col32(s);
    const int *drp_p = dP.rp32.p, *dcol_p = dP.col32.p;
    const double* dval_p = dP.val.p;
    keys_out.alloc(nnz);
    idx_in.alloc(nnz);
    idx_out.alloc(nnz);
    rowof.alloc(nnz);
    launch_rows(s, nnz, iota_kernel, (int)nnz, idx_in.p);
    launch_rows(s, n, expand_rows_kernel, drp_p, (int)n, rowof.p);
    sort_pairs_stable(s, dcol_p, keys_out.p, idx_in.p, idx_out.p, (int)nnz, nc, tmp);
    rcol.alloc(nnz);
    rval.alloc(nnz);
    launch_rows(s, nnz, gather_transpose_kernel, (int)nnz, idx_out.p, rowof.p, dval_p, rcol.p, rval.p);
    cnt.alloc((size_t)nc + 1);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int) * cnt.n, s));
    launch_rows(s, nnz, count_cols_kernel, (int)nnz, dcol_p, cnt.p);
    rrp.alloc((size_t)nc + 1);
    exclusive_scan(s, cnt.p, rrp.p, (int)nc, tmp);
    HIP_CHECK(hipGetLastError());
    R = HostCSR();
    R.n_global_rows = nc;
    R.n_global_cols = P.n_global_rows;
    R.row_starts = P.col_starts;
    R.col_starts = P.row_starts;
    std::vector<int> hrp = download_ints(s, rrp.p, nc + 1);
    R.rp.assign(hrp.begin(), hrp.end());
    R.col.resize(nnz);
    R.val.resize(nnz);
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 columns");
    copy_to_host(R.col.data(), rcol.p, sizeof(long long) * nnz, s);
    copy_to_host(R.val.data(), rval.p, sizeof(double) * nnz, nullptr);
    if (imgs) {  // R where it was computed, for the Galerkin product
        std::unique_ptr<DevCsr> d(new DevCsr());
        d->rp32 = std::move(rrp);
        d->col64 = std::move(rcol);
        d->val = std::move(rval);
        imgs->put(R, std::move(d));
    }
    return true;
}

}  // namespace amg
