// par_matrix.hip -- ParCSRMatrix on the GPU.
//
// Layout in HBM: rank-local rows, int32 row_ptr, int32 column ids
// renumbered [0, n_cols_local) local | [n_cols_local, +n_halo) halo, fp64 values, fp64
// 1/a_ii.  Columns stay in ascending GLOBAL order inside a row, so row sums are identical
// for any partition.  Row blocks are split into "interior" (no halo column) and
// "boundary" lists: the interior kernel runs while RCCL moves the halo on a second
// stream; the boundary kernel runs after the halo event.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "device.hpp"

namespace amg {

// Zero-filled host staging buffer, written in parallel: std::vector's value-initialising
// constructor zeroes on one thread (0.1-0.2 s for the 1-2 GB of a 256^3 level's streams)
template <class T>
struct ParZeros {
    std::unique_ptr<T[]> p;
    size_t n = 0;
    explicit ParZeros(size_t count) : p(new T[count > 0 ? count : 1]), n(count) {
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < (int64_t)count; ++i) p[i] = T();
    }
    T* data() { return p.get(); }
    const T* data() const { return p.get(); }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
    T* begin() { return p.get(); }
};

// ---- staged host <-> device copies (device.hpp) ----------------------------------------
namespace {

constexpr size_t kStageChunk = size_t(32) << 20;

// two pinned chunks + a copy stream per (device, user); kept for the process lifetime
struct Stage {
    int device = -1;
    bool busy = false;
    hipStream_t s = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    char* buf[2] = {nullptr, nullptr};
};

std::mutex g_stage_mu;
std::vector<Stage*> g_stages;

Stage* stage_acquire() {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_stage_mu);
    for (Stage* st : g_stages)
        if (!st->busy && st->device == dev) {
            st->busy = true;
            return st;
        }
    std::unique_ptr<Stage> st(new Stage());
    st->device = dev;
    HIP_CHECK(hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        HIP_CHECK(hipEventCreateWithFlags(&st->ev[b], hipEventDisableTiming));
        HIP_CHECK(hipHostMalloc((void**)&st->buf[b], kStageChunk, hipHostMallocDefault));
    }
    st->busy = true;
    g_stages.push_back(st.get());
    return st.release();
}

void stage_release(Stage* st) {
    std::lock_guard<std::mutex> g(g_stage_mu);
    st->busy = false;
}

struct StageLease {
    Stage* st;
    StageLease() : st(stage_acquire()) {}
    ~StageLease() { stage_release(st); }
};

void par_memcpy(void* dst, const void* src, size_t bytes) {
    const int64_t parts = (int64_t)std::max<size_t>(1, bytes >> 21);  // 2 MiB pieces
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < parts; ++q) {
        const size_t a = bytes * (size_t)q / (size_t)parts, b = bytes * (size_t)(q + 1) / (size_t)parts;
        std::memcpy((char*)dst + a, (const char*)src + a, b - a);
    }
}

}  // namespace

void copy_to_device(void* dst, const void* src, size_t bytes) {
    if (bytes < (size_t(4) << 20)) {
        if (bytes) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return;
    }
    StageLease L;
    Stage& S = *L.st;
    size_t c = 0;
    for (size_t off = 0; off < bytes; off += kStageChunk, ++c) {
        const int b = (int)(c & 1);
        const size_t len = std::min(kStageChunk, bytes - off);
        if (c >= 2) HIP_CHECK(hipEventSynchronize(S.ev[b]));  // the DMA out of this buffer is done
        par_memcpy(S.buf[b], (const char*)src + off, len);
        HIP_CHECK(hipMemcpyAsync((char*)dst + off, S.buf[b], len, hipMemcpyHostToDevice, S.s));
        HIP_CHECK(hipEventRecord(S.ev[b], S.s));
    }
    HIP_CHECK(hipStreamSynchronize(S.s));
}

void copy_to_host(void* dst, const void* src, size_t bytes, hipStream_t after) {
    if (after) HIP_CHECK(hipStreamSynchronize(after));
    if (bytes < (size_t(4) << 20)) {
        if (bytes) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return;
    }
    StageLease L;
    Stage& S = *L.st;
    const size_t nc = (bytes + kStageChunk - 1) / kStageChunk;
    auto issue = [&](size_t c) {
        const size_t off = c * kStageChunk, len = std::min(kStageChunk, bytes - off);
        HIP_CHECK(hipMemcpyAsync(S.buf[c & 1], (const char*)src + off, len, hipMemcpyDeviceToHost, S.s));
        HIP_CHECK(hipEventRecord(S.ev[c & 1], S.s));
    };
    issue(0);
    for (size_t c = 0; c < nc; ++c) {
        if (c + 1 < nc) issue(c + 1);  // into the other buffer, emptied in the previous round
        HIP_CHECK(hipEventSynchronize(S.ev[c & 1]));
        const size_t off = c * kStageChunk, len = std::min(kStageChunk, bytes - off);
        par_memcpy((char*)dst + off, S.buf[c & 1], len);
    }
}

Context::~Context() {
    loopback_leave(*this);
    if (nccl) (void)ncclCommDestroy(nccl);
    if (ev_pack) (void)hipEventDestroy(ev_pack);
    if (ev_halo) (void)hipEventDestroy(ev_halo);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

// Row blocks of the CSR-stream kernel: <= kCAP nonzeros, <= kTPB rows, one class (interior /
// boundary), and <= kCAP / lw distinct lines of x (lw = 8 or 4 doubles; local lines first,
// then halo lines).  Each block gets its sorted line list ("x tile") and every nonzero a
// 16-bit index into the tile: slot * lw + (column mod lw).  A single row touching more lines
// than a tile holds becomes a block of its own and takes the untiled path.
struct BlockBuild {
    std::vector<int2> blocks;     // interior all-templated, other interior, then boundary blocks
    std::vector<int> tile_ptr;    // nb + 1
    std::vector<int> tile_lines;  // global line ids per block
    hvec<uint16_t> lcol;          // per nonzero (nnz + kPad)
    int nb_int = 0, nb_bnd = 0, nb_skip = 0;  // nb_skip: leading interior all-templated blocks
};

// tplf (optional): per row 1 = handled by the template kernel; blocks then also break where it
// changes, and all-templated interior blocks come first
// sample > 1: cut only every sample-th chunk (statistics for the format choices below; no
// tile indices)
static BlockBuild build_row_blocks(const std::vector<int>& rp, const hvec<int>& col,
                                   const std::vector<uint8_t>& cls, int64_t ncl, int64_t nhalo,
                                   const std::vector<uint8_t>* tplf = nullptr, int row_cap = kTPB,
                                   bool line_cap = true, bool want_lcol = true, int lw = 8, int sample = 1,
                                   int unit = 1) {
    // unit > 1 (an operator with a segment row map): blocks start and end on multiples of
    // `unit` rows, and the caps are tested a whole segment at a time
    AMG_ASSERT(unit >= 1 && (unit == 1 || tplf == nullptr));
    if (sample > 1) want_lcol = false;
    const int n = (int)rp.size() - 1;
    const int sh = lw == 8 ? 3 : 2, tl_cap = kCAP / lw;
    AMG_ASSERT(lw == 8 || lw == 4);
    const int64_t hl0 = (ncl + lw - 1) / lw;
    auto line_of = [&](int c) -> int64_t { return c < ncl ? c >> sh : hl0 + ((c - ncl) >> sh); };
    struct Rec {
        int r0, r1;
        std::vector<int> lines;
        bool bnd, tpl;
    };
    BlockBuild out;
    // every entry below col.size() is written by the block that holds it; the pad is zero.
    // want_lcol = false: the tile indices are built on the device (formats.hip)
    if (want_lcol) {
        out.lcol.resize(col.size() + kPad);
        std::fill(out.lcol.begin() + (int64_t)(rp.back()), out.lcol.end(), (uint16_t)0);
    }
    // The greedy cut runs independently on a fixed number of row chunks (each chunk starts a
    // block at its first row), in parallel: blocks never change the arithmetic (rows never
    // straddle a block), and a fixed chunk count keeps the cut independent of the thread count.
    // Sequential, the cut took 0.4-0.7 s per 256^3-level operator.
    // (r5: also operators of few but long rows -- sa27's R1, 49,492 rows of ~270 entries, took
    // 0.45 s in one chunk)
    const int nch = n >= (1 << 16) || (n >= (1 << 12) && rp.back() >= (1 << 20)) ? 64 : 1;
    std::vector<std::vector<Rec>> recs((size_t)nch);
    // Each thread keeps the open block's lines (and the current row's new ones) in an
    // open-addressing table with a generation per slot: a slot of an older generation (block)
    // reads as empty, so closing a block clears nothing.  Sized for one block's lines (<= its
    // entries: kCAP, or one longer row) plus one row's.  r5: per-thread arrays indexed by line
    // id (16 B per line of the column space, filled per call) cost more than the cut itself on
    // level-0 operators (0.54 s for a 16.7 M-column operator on 16 threads).
    int max_row = 0;
#pragma omp parallel for reduction(max : max_row) schedule(static)
    for (int i = 0; i < n; ++i) max_row = std::max(max_row, rp[i + 1] - rp[i]);
    int hb = 10;
    while (((size_t)1 << hb) < 2 * ((size_t)kCAP + 2 * (size_t)max_row * (size_t)unit)) ++hb;
    const size_t H = (size_t)1 << hb;
#pragma omp parallel if (nch > 1)
    {
        std::vector<int64_t> hkey(H), hrow(H);
        std::vector<int> hgen(H, -1), hpos(H);
        std::vector<char> hin(H);
        std::vector<int> lines, cand;
        std::vector<size_t> cslot;
        int blk = 0;  // per thread, never reset: generations stay unique across chunks
        size_t used = 0;
        // the slot of line L in the open block's generation (inserted: not in the block, no row)
        auto find = [&](int64_t L) -> size_t {
            size_t h = (size_t)(((uint64_t)L * 0x9E3779B97F4A7C15ull) >> (64 - hb));
            for (;;) {
                if (hgen[h] != blk) {
                    AMG_ASSERT(++used < H);
                    hgen[h] = blk;
                    hkey[h] = L;
                    hin[h] = 0;
                    hrow[h] = -1;
                    return h;
                }
                if (hkey[h] == L) return h;
                h = (h + 1) & (H - 1);
            }
        };
        auto next_block = [&] {
            ++blk;
            used = 0;
        };
#pragma omp for schedule(dynamic, 1)
        for (int ch = 0; ch < nch; ++ch) {
            if (ch % sample) continue;
            const int ra = (int)((int64_t)n * ch / nch) / unit * unit;
            const int rb = ch + 1 == nch ? n : (int)((int64_t)n * (ch + 1) / nch) / unit * unit;
            std::vector<Rec>& rc = recs[(size_t)ch];
            int r0 = ra, nl = 0;
            long long acc = 0;
            lines.clear();
            next_block();
            auto emit = [&](int a, int b) {
                if (b <= a) return;
                std::sort(lines.begin(), lines.end());
                for (size_t q = 0; q < lines.size(); ++q) hpos[find(lines[q])] = (int)q;
                const bool tiled = (int)lines.size() <= tl_cap;
                if (want_lcol)
                    for (int k = rp[a]; k < rp[b]; ++k) {
                        const int c = col[k];
                        // element within its line
                        const int e = c < ncl ? (c & (lw - 1)) : (int)((c - ncl) & (lw - 1));
                        out.lcol[k] = tiled ? (uint16_t)(hpos[find(line_of(c))] * lw + e) : (uint16_t)0;
                    }
                rc.push_back({a, b, tiled ? lines : std::vector<int>(), cls[a] != 0,
                              tplf != nullptr && (*tplf)[a] != 0});
                if (!tiled) rc.back().lines.assign(tl_cap + 1, 0);  // marker: untiled
                lines.clear();
                next_block();
            };
            // distinct lines of rows [r, r + unit) not yet in the open block (marker keeps them
            // distinct per call)
            auto collect = [&](int r, int64_t marker) {
                cand.clear();
                cslot.clear();
                for (int k = rp[r]; k < rp[std::min(r + unit, rb)]; ++k) {
                    const int64_t L = line_of(col[k]);
                    const size_t h = find(L);
                    if (!hin[h] && hrow[h] != marker) {
                        hrow[h] = marker;
                        cand.push_back((int)L);
                        cslot.push_back(h);
                    }
                }
            };
            for (int r = ra; r < rb; r += unit) {
                const long long len = rp[std::min(r + unit, rb)] - rp[r];
                collect(r, 2 * (int64_t)r);
                if (r > r0 && (cls[r] != cls[r0] || acc + len > kCAP || r - r0 + unit > row_cap ||
                               (line_cap && nl + (int)cand.size() > tl_cap) ||
                               (tplf && (*tplf)[r] != (*tplf)[r0]))) {
                    emit(r0, r);  // closes [r0, r); a new generation
                    r0 = r;
                    acc = 0;
                    nl = 0;
                    collect(r, 2 * (int64_t)r + 1);  // all of row r's lines are new to the new block
                }
                for (size_t q = 0; q < cand.size(); ++q) {
                    hin[cslot[q]] = 1;
                    lines.push_back(cand[q]);
                }
                nl += (int)cand.size();
                acc += len;
            }
            emit(r0, rb);
        }
    }
    for (int pass = 0; pass < 3; ++pass)
        for (const std::vector<Rec>& rc : recs)
            for (const Rec& R : rc) {
                const int p = R.bnd ? 2 : R.tpl ? 0 : 1;
                if (p != pass) continue;
                out.blocks.push_back(make_int2(R.r0, R.r1));
                out.tile_ptr.push_back((int)out.tile_lines.size());
                out.tile_lines.insert(out.tile_lines.end(), R.lines.begin(), R.lines.end());
                (pass == 2 ? out.nb_bnd : out.nb_int)++;
                if (pass == 0) out.nb_skip++;
            }
    out.tile_ptr.push_back((int)out.tile_lines.size());
    return out;
}

// Value-indexed CSR (Kourtis et al., CF'08): blocks whose nonzeros take <= 256 distinct
// values (exact bit patterns) get a table of those values and a 1-byte index per nonzero,
// lane-major like the tile indices (entry j of the block -> lane j % kTPB, slot j / kTPB).
// Returns per-block table offset (-1: value stream) and table size for the block headers.
// For square operators also the table index of each row's diagonal (dvi, 1 byte per row) and
// per block whether every row has one (then Jacobi forms 1 / a_ii from the table in-kernel
// instead of streaming dinv: 1 byte per row instead of 8).
// Lane-major position of entry j of a block whose lanes hold nu entries each, as pairs:
// entry j = 512 p + 2 t + h sits at lane t, slot 2 p + h (p < nu / 2).
static inline size_t lane_pos(int j, int nu) {
    return (size_t)((j & (2 * kTPB - 1)) >> 1) * (size_t)nu + 2 * (size_t)(j / (2 * kTPB)) + (size_t)(j & 1);
}

// Index layout.  Square operators (x-tile kernel, 8 slots, entry pairs: lane_pos): kCAP
// bytes per block at bid * kCAP.  Rectangular ones (gather kernel, entry j at lane j % kTPB,
// slot j / kTPB): NU = 2, 4 or 8 slots by block size (the kernel's choice), packed, block
// offset in vofs (header field 0, unused by the gather kernel otherwise).
static int gather_slots(int nz) { return nz > 4 * kTPB ? 8 : nz > 2 * kTPB ? 4 : 2; }

static void build_value_index(DevMatrix& M, const HostCSR& H, const std::vector<int>& hrp, const BlockBuild& bb,
                              std::vector<int>& vt_off, std::vector<int>& vt_len,
                              std::vector<uint8_t>& dvi, std::vector<char>& dvi_ok,
                              std::vector<int64_t>& vofs) {
    const size_t nbk = bb.blocks.size();
    PhaseTimer tm(M.ctx->host);
    std::vector<std::vector<uint64_t>> tabs(nbk);
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t q = 0; q < nbk; ++q) {
        const int kb = hrp[bb.blocks[q].x], nz = hrp[bb.blocks[q].y] - kb;
        if (nz > kCAP || nz == 0) continue;
        std::vector<uint64_t> t(nz);
        std::memcpy(t.data(), H.val.data() + kb, sizeof(double) * (size_t)nz);
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        if (t.size() <= 256) tabs[q] = std::move(t);
    }
    tm.lap("      vi: per-block sort / unique");
    std::vector<int> ptr(std::max<size_t>(nbk, 1), -1);
    int64_t total = 0, vin = 0;
    int nvi = 0;
    for (size_t q = 0; q < nbk; ++q)
        if (!tabs[q].empty()) {
            ptr[q] = (int)total;
            total += (int64_t)tabs[q].size();
            vin += hrp[bb.blocks[q].y] - hrp[bb.blocks[q].x];
            ++nvi;
        }
    M.n_vi_blocks = nvi;
    M.vi_nnz = vin;
    vt_off.assign(nbk, -1);
    vt_len.assign(nbk, 0);
    dvi.assign(M.square ? (size_t)M.n_rows + 1 : 0, 0);
    dvi_ok.assign(nbk, 0);
    for (size_t q = 0; q < nbk; ++q)
        if (!tabs[q].empty()) vt_off[q] = ptr[q], vt_len[q] = (int)tabs[q].size();
    if (nvi == 0) {
        M.vtab.reset();
        M.vidx.reset();
        return;
    }
    AMG_CHECK(total < INT_MAX, "value tables too large");
    std::vector<double> tab((size_t)total);
    vofs.assign(nbk + 1, 0);
    for (size_t q = 0; q < nbk; ++q) {
        const int nz = hrp[bb.blocks[q].y] - hrp[bb.blocks[q].x];
        vofs[q + 1] = vofs[q] + (M.tiled ? kCAP : tabs[q].empty() ? 0 : gather_slots(nz) * kTPB);
    }
    AMG_CHECK(vofs[nbk] < INT_MAX, "value index stream too large");
    ParZeros<uint8_t> idx((size_t)vofs[nbk] + 16);
    tm.lap("      vi: offsets");
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t q = 0; q < nbk; ++q) {
        if (tabs[q].empty()) continue;
        const std::vector<uint64_t>& t = tabs[q];
        std::memcpy(tab.data() + ptr[q], t.data(), sizeof(double) * t.size());
        const int kb = hrp[bb.blocks[q].x], nz = hrp[bb.blocks[q].y] - kb;
        for (int j = 0; j < nz; ++j) {
            uint64_t bits;
            std::memcpy(&bits, H.val.data() + kb + j, sizeof(bits));
            const size_t at = std::lower_bound(t.begin(), t.end(), bits) - t.begin();
            // square (x-tile kernel): entry pairs; rectangular (gather kernel): entry j at
            // lane j % kTPB, slot j / kTPB, NU slots per lane
            const size_t pos = M.tiled ? lane_pos(j, kCAP / kTPB)
                                        : (size_t)(j % kTPB) * gather_slots(nz) + (size_t)(j / kTPB);
            idx[(size_t)vofs[q] + pos] = (uint8_t)at;
        }
        if (!M.square) continue;
        bool ok = true;
        for (int r = bb.blocks[q].x; r < bb.blocks[q].y; ++r) {
            int64_t k = H.rp[r], e = H.rp[r + 1];
            const int64_t g = M.first_row + r;
            while (k < e && H.col[k] < g) ++k;
            if (k == e || H.col[k] != g || H.val[k] == 0.0) {
                ok = false;
                continue;
            }
            uint64_t bits;
            std::memcpy(&bits, H.val.data() + k, sizeof(bits));
            dvi[r] = (uint8_t)(std::lower_bound(t.begin(), t.end(), bits) - t.begin());
        }
        dvi_ok[q] = ok;
    }
    tm.lap("      vi: indices + diagonal table slots");
    M.vtab.upload(tab.data(), tab.size());
    M.vidx.upload(idx.data(), idx.size());
    tm.lap("      vi: upload");
}


// Row templates.  A row qualifies when all its columns are local and it has
// 1..kTplMaxLen entries; its key is (column - row offsets, value bits, 1/a_ii bits).  Rows
// with equal keys share a template.  Each thread scans a contiguous chunk into a local
// dictionary; the chunk dictionaries merge in chunk order into <= kTplMax templates of
// <= kTplEntries entries (later shapes beyond either cap stay untemplated).
struct TplBuild {
    std::vector<uint8_t> id;  // per row, kTplNone = not templated
    std::vector<int> hdr, off;
    std::vector<double> val, pd;
    int64_t rows = 0;
};

static TplBuild build_templates(const std::vector<int>& rp, const hvec<int>& col,
                                const hvec<double>& val, const std::vector<double>& dinv,
                                int64_t ncl) {
    const int n = (int)rp.size() - 1;
    TplBuild T;
    T.id.assign((size_t)n, (uint8_t)kTplNone);
    if (n <= 0) return T;
    auto bits = [](double v) {
        uint64_t u;
        std::memcpy(&u, &v, sizeof(u));
        return u;
    };
    auto qualifies = [&](int r) {
        const int len = rp[r + 1] - rp[r];
        if (len <= 0 || len > kTplMaxLen) return false;
        for (int k = rp[r]; k < rp[r + 1]; ++k)
            if (col[k] >= ncl) return false;
        return true;
    };
    auto key_hash = [&](int r) {
        uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(rp[r + 1] - rp[r] + 1);
        auto mix = [&](uint64_t v) {
            h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h *= 0xBF58476D1CE4E5B9ull;
        };
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            mix((uint64_t)(uint32_t)(col[k] - r));
            mix(bits(val[k]));
        }
        mix(bits(dinv[r]));
        return h;
    };
    auto same = [&](int a, int b) {
        const int la = rp[a + 1] - rp[a];
        if (la != rp[b + 1] - rp[b] || bits(dinv[a]) != bits(dinv[b])) return false;
        for (int k = 0; k < la; ++k)
            if (col[rp[a] + k] - a != col[rp[b] + k] - b || bits(val[rp[a] + k]) != bits(val[rp[b] + k]))
                return false;
        return true;
    };
    // quick rejection (Galerkin coarse operators: nearly every row is its own shape): when
    // 4096 rows spread over the operator already show more than 2 kTplMax distinct keys,
    // the templates could not cover half the rows -- skip the full scan
    if (n > 65536) {
        std::vector<uint64_t> sk;
        for (int t = 0; t < 4096; ++t) {
            const int r = (int)((int64_t)n * t / 4096);
            if (qualifies(r)) sk.push_back(key_hash(r));
        }
        std::sort(sk.begin(), sk.end());
        sk.erase(std::unique(sk.begin(), sk.end()), sk.end());
        if ((int)sk.size() > 2 * kTplMax) return T;
    }
    const int nch = std::max(1, std::min(256, n / 16384));
    std::vector<std::vector<int>> reps(nch);       // representative row per local template
    std::vector<std::vector<uint64_t>> hashes(nch);
    std::vector<int16_t> lid((size_t)n, -1);
#pragma omp parallel for schedule(dynamic, 1)
    for (int c = 0; c < nch; ++c) {
        const int r0 = (int)((int64_t)n * c / nch), r1 = (int)((int64_t)n * (c + 1) / nch);
        std::unordered_map<uint64_t, std::vector<int>> m;
        std::vector<int>& R = reps[c];
        int last = -1;
        for (int r = r0; r < r1; ++r) {
            if (!qualifies(r)) continue;
            if (last >= 0 && same(R[last], r)) {
                lid[r] = (int16_t)last;
                continue;
            }
            const uint64_t h = key_hash(r);
            int found = -1;
            auto it = m.find(h);
            if (it != m.end())
                for (int t : it->second)
                    if (same(R[t], r)) {
                        found = t;
                        break;
                    }
            if (found < 0) {
                if ((int)R.size() >= kTplMax) continue;
                found = (int)R.size();
                R.push_back(r);
                hashes[c].push_back(h);
                m[h].push_back(found);
            }
            lid[r] = (int16_t)found;
            last = found;
        }
    }
    // merge (chunk order) into the global dictionary
    std::vector<std::vector<int>> gmap(nch);
    std::vector<int> grep;
    std::unordered_map<uint64_t, std::vector<int>> gm;
    int ent = 0;
    for (int c = 0; c < nch; ++c) {
        gmap[c].assign(reps[c].size(), -1);
        for (size_t t = 0; t < reps[c].size(); ++t) {
            const int r = reps[c][t];
            const uint64_t h = hashes[c][t];
            int g = -1;
            auto it = gm.find(h);
            if (it != gm.end())
                for (int q : it->second)
                    if (same(grep[q], r)) {
                        g = q;
                        break;
                    }
            const int len4 = (rp[r + 1] - rp[r] + 3) & ~3;  // padded run (below)
            if (g < 0 && (int)grep.size() < kTplMax && ent + len4 <= kTplEntries) {
                g = (int)grep.size();
                grep.push_back(r);
                gm[h].push_back(g);
                ent += len4;
            }
            gmap[c][t] = g;
        }
    }
    int64_t rows = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : rows)
    for (int c = 0; c < nch; ++c) {
        const int r0 = (int)((int64_t)n * c / nch), r1 = (int)((int64_t)n * (c + 1) / nch);
        for (int r = r0; r < r1; ++r)
            if (lid[r] >= 0 && gmap[c][lid[r]] >= 0) {
                T.id[r] = (uint8_t)gmap[c][lid[r]];
                ++rows;
            }
    }
    T.rows = rows;
    for (int r : grep) {
        const int start = (int)T.off.size(), len = rp[r + 1] - rp[r];
        int dk = 255;
        for (int k = 0; k < len; ++k) {
            T.off.push_back(col[rp[r] + k] - r);
            T.val.push_back(val[rp[r] + k]);
            if (col[rp[r] + k] == r && dk == 255) dk = k;
        }
        // runs start at multiples of 4 entries: the window kernels read 4 slots (16 bytes) and
        // 2 x 2 values per LDS instruction; padding repeats the run's first slot with value 0
        // and is never summed (entries >= len are masked)
        for (int k = len; k & 3; ++k) {
            T.off.push_back(col[rp[r]] - r);
            T.val.push_back(0.0);
        }
        T.hdr.push_back(start | len << 16 | (int)((unsigned)dk << 24));
        T.pd.push_back(dinv[r]);
    }
    return T;
}

// The environment's build knobs, read once at the top of build_view and of
// ensure_gs_blocks -- per build, not per process: tests change them between builds -- so that
// every stage below is a function of its arguments.  The launch-time knobs
// (AMG_KERNEL_VARIANT, AMG_GATHER_C16, AMG_TPL_MARCH_CHUNKS) are read by the launchers.
struct BuildKnobs {
    int64_t tpl_min_rows = 16384;  // AMG_TPL_MIN_ROWS: rows from which half-templated operators take templates
    int rect_tile = -1;            // AMG_RECT_TILE=0 / 1: rectangular operators never / always on x tiles
    int tile_line = 0;             // AMG_TILE_LINE=8 / 4: forces the x-tile line width (doubles)
    bool trace_blocks = false;     // AMG_TRACE_BLOCKS: print the block statistics of every build
    bool tpl_master = true;        // AMG_TPL_MASTER=0: no uniform-stencil master
    bool gs_templates = true;      // AMG_GS_TEMPLATES=0: no GS templates
    bool gs_split = true;          // AMG_GS_SPLIT=0: no split sweeps
    int64_t gs_split_npr = 12;     // AMG_GS_SPLIT_NPR: entries per row from which sweeps split
};

static BuildKnobs read_build_knobs() {
    BuildKnobs k;
    auto off = [](const char* name) {
        const char* e = std::getenv(name);
        return e && std::atoi(e) == 0;
    };
    if (const char* e = std::getenv("AMG_TPL_MIN_ROWS")) k.tpl_min_rows = std::atoll(e);
    if (const char* e = std::getenv("AMG_RECT_TILE")) k.rect_tile = std::atoi(e);
    if (const char* e = std::getenv("AMG_TILE_LINE")) k.tile_line = std::atoi(e);
    k.trace_blocks = std::getenv("AMG_TRACE_BLOCKS") != nullptr;
    k.tpl_master = !off("AMG_TPL_MASTER");
    k.gs_templates = !off("AMG_GS_TEMPLATES");
    k.gs_split = !off("AMG_GS_SPLIT");
    if (const char* e = std::getenv("AMG_GS_SPLIT_NPR")) k.gs_split_npr = std::atoll(e);
    return k;
}

// Uniform stencil: a constant-coefficient stencil's boundary templates are
// its interior template with entries removed.  When the longest template (the master) has a
// kernel instantiation (7 or 27 entries) and every template's (offset, value bits) entries are
// a subsequence of the master's -- in order, since offsets ascend -- and holds the master's
// diagonal with the same 1/a_ii, a row is (master, entry mask): the kernels take values and
// window slots from kernel arguments and skip the entries a row lacks.  The products and their
// order are the row's own, so results are unchanged (bit-identical).
static TplFormat::Master find_master_template(const TplBuild& tb, const std::vector<int>& ldo) {
    TplFormat::Master m;
    const int nt = (int)tb.hdr.size();
    if (nt == 0) return m;
    auto start = [&](int t) { return tb.hdr[t] & 0xffff; };
    auto len = [&](int t) { return (tb.hdr[t] >> 16) & 0xff; };
    auto diag = [&](int t) { return (int)((unsigned)tb.hdr[t] >> 24); };
    auto bits = [](double v) {
        uint64_t u;
        std::memcpy(&u, &v, sizeof(u));
        return u;
    };
    int M = 0;
    for (int t = 1; t < nt; ++t)
        if (len(t) > len(M)) M = t;
    const int ne = len(M);
    if ((ne != 7 && ne != 27) || diag(M) == 255) return m;
    const int sm = start(M);
    std::vector<unsigned> mask(nt, 0u);
    for (int t = 0; t < nt; ++t) {
        if (diag(t) == 255 || bits(tb.pd[t]) != bits(tb.pd[M])) return m;
        int e = 0;
        for (int k = 0; k < len(t); ++k) {
            const int o = tb.off[start(t) + k];
            while (e < ne && tb.off[sm + e] != o) ++e;
            if (e == ne || bits(tb.val[start(t) + k]) != bits(tb.val[sm + e])) return m;
            mask[t] |= 1u << e;
            ++e;
        }
        if (!(mask[t] >> diag(M) & 1u)) return m;
    }
    m.ne = ne;
    m.diag = diag(M);
    m.pd = tb.pd[M];
    for (int e = 0; e < ne; ++e) {
        m.slot.push_back(ldo[sm + e]);
        m.val.push_back(tb.val[sm + e]);
        if (tb.off[sm + e] == -1) m.em = e;
        if (tb.off[sm + e] == 1) m.ep = e;
    }
    m.mask.upload(mask.data(), mask.size());
    m.mask_host = std::move(mask);
    return m;
}

void DevMatrix::build(Context* c, HostCSR&& h, bool replicated_view) {
    build_view(c, h, replicated_view);
    host = std::move(h);
}

void DevMatrix::defer(Context* c, HostCSR&& h) {
    ctx = c;
    replicated = false;
    host = std::move(h);
    const HostComm& comm = ctx->host;
    first_row = host.row_starts[comm.rank];
    n_rows = host.nrows();
    first_col = host.col_starts[comm.rank];
    n_cols_local = host.col_starts[comm.rank + 1] - first_col;
    nnz = host.nnz();
    square = host.n_global_rows == host.n_global_cols && host.row_starts == host.col_starts;
    deferred = true;
}

void DevMatrix::ensure_built() {
    if (!deferred) return;
    build_view(ctx, host);
    deferred = false;
}

// ---- the stages of DevMatrix::build_view, in the order it runs them.  H is the CSR being
// built from (the caller's: see build_view), hrp / hcol its int32 row pointers and local
// column numbers.

// Local column numbering [local | halo] and the boundary class of every row (1: the row
// touches a halo column).
static void local_columns(const HostCSR& H, const HaloPlan& plan, int64_t first_col, int64_t n_cols_local,
                          std::vector<int>& hrp, hvec<int>& hcol, std::vector<uint8_t>& cls) {
    const int64_t n_rows = H.nrows(), nnz = H.nnz();
    hrp.resize(n_rows + 1);
    // every entry written below; capacity for the kPad zero entries appended after the
    // templates, so that resize does not reallocate and copy (0.4 s for a 449 M-entry operator)
    hcol.reserve((size_t)nnz + kPad);
    hcol.resize(nnz);
    cls.assign(n_rows, 0);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i <= n_rows; ++i) hrp[i] = (int)H.rp[i];
    const int64_t clo = first_col, chi = first_col + n_cols_local;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; ++i) {
        uint8_t b = 0;
        for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k) {
            const int64_t g = H.col[k];
            if (g >= clo && g < chi) {
                hcol[k] = (int)(g - clo);
            } else {
                hcol[k] = (int)(n_cols_local + plan.find(g));
                b = 1;
            }
        }
        cls[i] = b;
    }
}

// Row templates: square operators whose templates cover every row, or at least half of
// the rows of a large operator (AMG_TPL_MIN_ROWS, default 16384; tests lower it).  Empty: none.
static TplBuild select_templates(const BuildKnobs& knobs, const HostCSR& H, const std::vector<int>& hrp,
                                 const hvec<int>& hcol, const std::vector<double>& di, int64_t n_cols_local) {
    const int64_t n_rows = H.nrows();
    TplBuild tb = build_templates(hrp, hcol, H.val, di, n_cols_local);
    const bool use = tb.rows == n_rows || (n_rows >= knobs.tpl_min_rows && 2 * tb.rows >= n_rows);
    if (!use) tb = TplBuild();
    return tb;
}

// The cut of an operator into row blocks: x tile or gather, and the x-tile line width.
struct CutChoice {
    bool tiled = false;
    int line_w = 8;
};

// The format choices (x tile or gather, 64- or 32-byte lines) read statistics of
// the 64-byte cut; r5 takes them from every 8th of its 64 row chunks (the whole
// operator below 65,536 rows) and cuts the operator once, at the chosen width.  Before,
// each choice cut the whole operator again: 0.6 s of sa27's setup.
static CutChoice choose_cut(const BuildKnobs& knobs, const std::vector<int>& hrp, const hvec<int>& hcol,
                            const std::vector<uint8_t>& cls, const std::vector<uint8_t>* tplf, int64_t n_cols_local,
                            int64_t n_halo, bool square, int gather_rpb, int unit = 1) {
    constexpr int kSample = 8;
    const BlockBuild s8 = build_row_blocks(hrp, hcol, cls, n_cols_local, n_halo, tplf, kTPB * gather_rpb, true,
                                           false, 8, kSample, unit);
    // rectangular operators take the x-tile kernel when their blocks reuse x lines: at most
    // 0.5 tile lines per nonzero.  Same-box A/B (profiles/r2y_rtile_*, r2z_rpb_*): 7-pt R0
    // 106 -> 79 us (0.23 lines / nnz), R1 66 -> 53 (0.34), P0 (4 rows per lane, 0.06)
    // 97 -> 80, P1 49 -> 39; sa27 P0 299 -> 234 (0.04), P1 33 -> 26; g3sub R0 24 -> 20
    // (0.33), P0 19 -> 15; sa27 R1 122 -> 158 at 0.70 (a 297-entry block loading 210
    // lines) stays on the gather kernel.
    // AMG_RECT_TILE=0 / 1: never / always (A/B runs)
    int64_t tile_lines_total = 0, tile_full = 0, sample_nnz = 0;
    for (size_t q = 0; q + 1 < s8.tile_ptr.size(); ++q) {
        const int nt = s8.tile_ptr[q + 1] - s8.tile_ptr[q];
        tile_lines_total += nt;
        tile_full += nt >= kTileLines;
        sample_nnz += hrp[s8.blocks[q].y] - hrp[s8.blocks[q].x];
    }
    CutChoice cut;
    const int mode = knobs.rect_tile;
    cut.tiled = square || (mode != 0 && (mode == 1 || 2 * tile_lines_total <= sample_nnz));
    if (knobs.trace_blocks) {
        const int64_t lines = tile_lines_total, full = tile_full;
        std::fprintf(stderr, "[amg-blocks] %s rows %lld cols %lld nnz %lld sampled: blocks %zu lines %lld full %lld nnz %lld rpb %d\n",
                     square ? "square" : cut.tiled ? "rect-tiled" : "rect-gather", (long long)hrp.size() - 1,
                     (long long)n_cols_local, (long long)hrp.back(), s8.blocks.size(), (long long)lines, (long long)full,
                     (long long)sample_nnz, gather_rpb);
    }
    // x-tile line width: operators whose blocks, cut at 256 lines of
    // 64 B, run close to the cap (>= 3/4 full on average: Galerkin operators,
    // restrictions) are cut at 512 lines of 32 B (the 7-pt 256^3 A2: 40,250 -> 25,615
    // blocks; R0: same-box 76 -> 70 us); P-like operators (few lines per block) keep
    // 64-byte lines and their 1 KiB of line ids per block (sa27 P0: 234 us at 64 B, 263 at
    // 32 B), and so do square operators the 32-byte cut saves < 20 % of the blocks (the
    // 7-pt A1: 50,573 -> 46,841 blocks ran 144 -> 149 us; A2: 40,281 -> 25,640 ran 125 ->
    // 102 us); restrictions gain either way (R0 91 -> 88 us at -9 %, R1 61 -> 52 at -33 %).
    // AMG_TILE_LINE=8 / 4 forces the width.
    if (cut.tiled && !s8.blocks.empty()) {
        const int force = knobs.tile_line;
        const bool tryhalf = force == 4 || (force != 8 && 4 * tile_lines_total >= 3 * (int64_t)kTileLines *
                                                                                     (int64_t)s8.blocks.size());
        if (tryhalf) {
            bool take = force == 4 || !square;
            if (!take) {
                const BlockBuild s4 = build_row_blocks(hrp, hcol, cls, n_cols_local, n_halo, tplf,
                                                       kTPB * gather_rpb, true, false, 4, kSample, unit);
                take = 5 * s4.blocks.size() <= 4 * s8.blocks.size();
            }
            if (take) cut.line_w = 4;
        }
    }
    return cut;
}

// The row templates on the device and their small table on the host.  Rows of blocks the CSR
// kernel still runs (blocks from bb.nb_skip on) are not the template kernel's.
static void upload_templates(TplFormat& T, TplBuild& tb, const BlockBuild& bb, int64_t n_rows) {
    std::vector<char> keep(n_rows, 0);
    for (int q = 0; q < bb.nb_skip; ++q)
        for (int r = bb.blocks[q].x; r < bb.blocks[q].y; ++r) keep[r] = 1;
    int64_t rows = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        if (!keep[i]) tb.id[i] = (uint8_t)kTplNone;
        rows += tb.id[i] != kTplNone;
    }
    T.rows = rows;
    T.n = (int)tb.hdr.size();
    T.n_ent = (int)tb.off.size();
    T.id.upload(tb.id.data(), tb.id.size());
    T.id_host = tb.id;
    T.hdr.upload(tb.hdr.data(), tb.hdr.size());
    T.off.upload(tb.off.data(), tb.off.size());
    T.val.upload(tb.val.data(), tb.val.size());
    T.pd.upload(tb.pd.data(), tb.pd.size());
    T.hdr_host = tb.hdr;
    T.off_host = tb.off;
    T.val_host = tb.val;
}

// x window: distinct offsets merged into bands while a gap is shorter than a workgroup's rows
// (a new band would load kTplRows more doubles than the gap); per entry its window slot.
// Returns the slots (empty, and T.win = 0, when the bands do not fit the window).
static std::vector<int> tpl_window(TplFormat& T, const TplBuild& tb) {
    std::vector<int> offs(tb.off);
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    std::vector<int2> bands;  // {lo, hi}
    for (int o : offs) {
        if (!bands.empty() && (int64_t)o - bands.back().y < kTplRows) bands.back().y = o;
        else bands.push_back(make_int2(o, o));
    }
    // even band starts and lengths: slot pairs map to 16-byte aligned pairs of x
    for (int2& bd : bands) bd.x &= ~1;
    auto blen = [](const int2& bd) { return (int64_t)(kTplRows + bd.y - bd.x + 1) & ~(int64_t)1; };
    int64_t w = 0;
    for (const int2& bd : bands) w += blen(bd);
    if ((int)bands.size() > kTplBands || w > kTplWin) return {};
    std::vector<int> ldo(tb.off.size());
    int base = 0;
    for (const int2& bd : bands) {
        T.blo.push_back(bd.x);
        T.bbase.push_back(base);
        base += (int)blen(bd);
    }
    T.wend = bands.back().x + (int)blen(bands.back());
    for (size_t k = 0; k < tb.off.size(); ++k) {
        const int o = tb.off[k];
        size_t q = 0;
        while (q + 1 < bands.size() && o > bands[q].y) ++q;
        ldo[k] = T.bbase[q] + (o - bands[q].x);
    }
    T.win = base;
    T.ldo.upload(ldo.data(), ldo.size());
    return ldo;
}

// z-marching: the shift D (a multiple of kTplRows, taken from the band starts) under which
// the most window slots of a block are slots of the block D rows back; used when at least a
// quarter of the window is reused.  Fills T.march_s and T.wsrc from T's window.
static void tpl_march(TplFormat& T, int64_t n_rows) {
    const int nbd = (int)T.blo.size(), base = T.win;
    auto reuse_map = [&](int64_t D, std::vector<int>* map) {
        int cnt = 0;
        for (int q = 0; q < nbd; ++q) {
            const int len = (q + 1 < nbd ? T.bbase[q + 1] : base) - T.bbase[q];
            for (int i = 0; i < len; ++i) {
                const int64_t g = D + T.blo[q] + i;  // relative to the old r0
                int src = -1;
                for (int q2 = 0; q2 < nbd && src < 0; ++q2) {
                    const int len2 = (q2 + 1 < nbd ? T.bbase[q2 + 1] : base) - T.bbase[q2];
                    const int64_t j = g - T.blo[q2];
                    if (j >= 0 && j < len2) src = T.bbase[q2] + (int)j;
                }
                if (map) (*map)[T.bbase[q] + i] = src;
                cnt += src >= 0;
            }
        }
        return cnt;
    };
    int64_t bestD = 0;
    int best = 0;
    std::vector<int64_t> cand;
    for (int q = 0; q < nbd; ++q) {
        cand.push_back(std::abs((int64_t)T.blo[q]));
        for (int q2 = q + 1; q2 < nbd; ++q2) cand.push_back((int64_t)T.blo[q2] - T.blo[q]);
    }
    for (int64_t D : cand) {
        D -= D % kTplRows;
        if (D <= 0 || D / kTplRows > INT_MAX / 2) continue;
        const int c = reuse_map(D, nullptr);
        if (c > best) best = c, bestD = D;
    }
    // 16-byte pair loads: an even row count keeps every pair inside or outside x
    if (bestD > 0 && 4 * best >= base && n_rows % 2 == 0) {
        std::vector<int> map(base, -1);
        reuse_map(bestD, &map);
        T.march_s = (int)(bestD / kTplRows);
        T.wsrc.upload(map.data(), map.size());
    }
}

// The per-nonzero streams of the CSR block kernels built on the host (AMG_DEVICE_FORMATS=0;
// formats.hip builds the same bytes on the GPU): block-aligned col / val, x-tile ids and tile
// indices, the value index and the row ends; fi gets what the block headers need.
static void host_block_streams(DevMatrix& M, PhaseTimer& tm, const HostCSR& H, const std::vector<int>& hrp,
                               const hvec<int>& hcol, const BlockBuild& bb, const std::vector<int64_t>& koff,
                               FormatHeaderInfo& fi) {
    const size_t nbk = bb.blocks.size();
    {
        ParZeros<int> cb((size_t)(koff[nbk] + kPad));
        ParZeros<double> vb(cb.size());
#pragma omp parallel for schedule(dynamic, 256)
        for (size_t q = 0; q < nbk; ++q) {
            const int kb = hrp[bb.blocks[q].x], nz = hrp[bb.blocks[q].y] - kb;
            std::copy(hcol.begin() + kb, hcol.begin() + kb + nz, cb.begin() + koff[q]);
            std::copy(H.val.begin() + kb, H.val.begin() + kb + nz, vb.begin() + koff[q]);
        }
        M.col.upload(cb.data(), cb.size());
        M.val.upload(vb.data(), vb.size());
    }
    if (M.tiled) {  // x tiles: the x-tile kernel only
        // x-tile line ids at a fixed stride (kCAP / line_w per block, padded with the block's
        // last line), so the kernel loads them without waiting for the block header
        const int tlb = kCAP / M.line_w;
        ParZeros<int> fx(std::max<size_t>(nbk, 1) * tlb);
#pragma omp parallel for schedule(static)
        for (size_t q = 0; q < nbk; ++q) {
            const int t0 = bb.tile_ptr[q], nt = bb.tile_ptr[q + 1] - t0;
            if (nt <= 0 || nt > tlb) continue;
            for (int j = 0; j < tlb; ++j)
                fx[q * tlb + j] = bb.tile_lines[t0 + std::min(j, nt - 1)];
        }
        M.tile_fixed.upload(fx.data(), fx.size());
        // lane-major per block (lane_pos): lane t's 8 indices are 16 contiguous bytes,
        // one 16-byte load per lane
        ParZeros<uint16_t> perm(std::max<size_t>(nbk, 1) * kCAP);
#pragma omp parallel for schedule(static)
        for (size_t q = 0; q < nbk; ++q) {
            const int kb = hrp[bb.blocks[q].x], nz = hrp[bb.blocks[q].y] - kb;
            if (nz > kCAP) continue;
            for (int j = 0; j < nz; ++j)
                perm[q * kCAP + lane_pos(j, kCAP / kTPB)] = bb.lcol[kb + j];
        }
        M.lcol.upload(perm.data(), perm.size());
    } else {
        M.tile_fixed.reset();
        M.lcol.reset();
    }
    tm.lap("    build: col / val / tile layouts");
    std::vector<uint8_t> hdvi;
    build_value_index(M, H, hrp, bb, fi.vt_off, fi.vt_len, hdvi, fi.dvi_ok, fi.vofs);
    if (M.n_vi_blocks > 0 && M.square) M.dvi.upload(hdvi.data(), hdvi.size());
    else M.dvi.reset();
    tm.lap("    build: value index");
    // per row: end of its nonzeros relative to its block's first (<= kCAP: 16 bits)
    std::vector<uint16_t> re((size_t)M.n_rows + 1, 0);
    for (size_t q = 0; q < nbk; ++q) {
        const int2 b = bb.blocks[q];
        if (hrp[b.y] - hrp[b.x] > kCAP) continue;
        for (int r = b.x; r < b.y; ++r) re[r] = (uint16_t)(hrp[r + 1] - hrp[b.x]);
    }
    M.rend.upload(re.data(), re.size());
}

// Gather operators: 16-bit column codes when every block's columns fit in <= 4
// bands of kGatherBand: a structured P / R block reads three
// planes' worth of columns, each a narrow band.  Lossless: the kernel decodes
// base[code >> 14] + (code & 0x3fff), the same column.  Left empty where a block does not fit.
static void gather_codes(const std::vector<int>& hrp, const hvec<int>& hcol, const std::vector<int2>& blocks,
                         const std::vector<int64_t>& koff, DevBuf<uint16_t>& col16, DevBuf<int4>& gband) {
    const size_t nbk = blocks.size();
    ParZeros<uint16_t> c16((size_t)(koff[nbk] + kPad));
    std::vector<int4> gb(nbk, make_int4(0, 0, 0, 0));
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : bad)
    for (size_t q = 0; q < nbk; ++q) {
        const int kb = hrp[blocks[q].x], nz = hrp[blocks[q].y] - kb;
        if (nz == 0 || nz > kCAP) continue;  // chunked path: int32 columns
        std::vector<int> u(hcol.begin() + kb, hcol.begin() + kb + nz);
        std::sort(u.begin(), u.end());
        int base[4] = {0, 0, 0, 0}, nbnd = 0;
        for (int c : u) {
            if (nbnd == 0 || c - base[nbnd - 1] >= kGatherBand) {
                if (nbnd == 4) {
                    nbnd = 5;
                    break;
                }
                base[nbnd++] = c;
            }
        }
        if (nbnd > 4) {
            ++bad;
            continue;
        }
        for (int t = nbnd; t < 4; ++t) base[t] = base[nbnd - 1];
        gb[q] = make_int4(base[0], base[1], base[2], base[3]);
        for (int j = 0; j < nz; ++j) {
            const int c = hcol[kb + j];
            int t = nbnd - 1;
            while (c < base[t]) --t;
            c16[koff[q] + j] = (uint16_t)((t << 14) | (c - base[t]));
        }
    }
    if (bad == 0) {
        col16.upload(c16.data(), c16.size());
        gband.upload(gb.data(), gb.size());
    }
}

// 32-byte block headers (two scalar loads per block):
//   {r0, r1, koff, nnz}, {diag slot, tile lines | dvi flag << 16, value-table offset (-1),
//   table size}
// diag slot (square operators): tile position of line r0 / line_w when the lines of the
// block's own rows are consecutive in its tile, so x[r] is read from the tile; else -1.
// Also M.jac_extra_all / jac_extra_csr: the Jacobi operand bytes of the CSR-kernel rows.
static std::vector<int4> block_headers(DevMatrix& M, const std::vector<int>& hrp, const BlockBuild& bb,
                                       const std::vector<int64_t>& koff, const FormatHeaderInfo& fi) {
    const size_t nbk = bb.blocks.size();
    const bool square = M.square, tiled = M.tiled;
    const int line_w = M.line_w;
    std::vector<int4> hh(std::max<size_t>(2 * nbk, 2), make_int4(0, 0, 0, 0));
    M.jac_extra_all = M.jac_extra_csr = 0;
    for (size_t q = 0; q < nbk; ++q) {
        const int2 b = bb.blocks[q];
        const int t0 = bb.tile_ptr[q], nt = bb.tile_ptr[q + 1] - t0;
        int dslot = -1;
        if (square && nt > 0 && nt <= kCAP / line_w) {
            const int ls = line_w == 8 ? 3 : 2;
            const int l0 = b.x >> ls, l1 = (b.y - 1) >> ls;
            const int* tl = bb.tile_lines.data() + t0;
            const int pos = (int)(std::lower_bound(tl, tl + nt, l0) - tl);
            bool ok = pos + (l1 - l0) < nt;
            for (int k = 0; ok && k <= l1 - l0; ++k) ok = tl[pos + k] == l0 + k;
            if (ok) dslot = pos;
        }
        hh[2 * q] = make_int4(b.x, b.y, (int)koff[q], hrp[b.y] - hrp[b.x]);
        if (square) {  // Jacobi operands beyond b: 1/a_ii (table index or fp64), x[r]
            const int64_t rows = b.y - b.x;
            const int64_t e = rows * (fi.dvi_ok[q] ? 1 : 8) + (dslot < 0 ? 8 * rows : 0);
            M.jac_extra_all += e;
            if ((int)q >= bb.nb_skip) M.jac_extra_csr += e;
        }
        // rectangular (gather) operators: field 0 = the block's offset in the VI index stream
        const int f0 = square ? dslot : tiled ? -1 : (fi.vofs.empty() ? 0 : (int)fi.vofs[q]);
        hh[2 * q + 1] = make_int4(f0, nt | (fi.dvi_ok[q] ? kHdrDvi : 0), fi.vt_off[q], fi.vt_len[q]);
    }
    return hh;
}

// Row map: block q's segments' vector rows at q * seg_stride(), padded with the last (the
// kernel loads them by block id alone, like the tile line ids).  Built on the host for both
// format builders: 4 bytes per segment.
static void upload_block_segments(DevMatrix& M, const std::vector<int2>& blocks) {
    const int S = M.row_seg, st = M.seg_stride();
    std::vector<int> sg(std::max<size_t>(blocks.size(), 1) * st, 0);
    for (size_t q = 0; q < blocks.size(); ++q) {
        const int s0 = blocks[q].x / S, ns = (blocks[q].y - blocks[q].x) / S;
        AMG_ASSERT(ns >= 1 && ns <= st && blocks[q].x % S == 0 && blocks[q].y % S == 0);
        for (int j = 0; j < st; ++j) sg[q * st + j] = M.seg_rows[s0 + std::min(j, ns - 1)];
    }
    M.seg.upload(sg.data(), sg.size());
}

// Format bytes of one default-variant SpMV (the kernel reads every lane slot of the
// fixed-stride streams, so their padding counts) into M.csr_fmt_bytes / M.spmv_fmt_bytes.
// With templates: the skipped blocks cost nothing; template rows cost 1 byte (id); the
// table (offsets, values, headers, 1/a_ii) is read from HBM once -- every further
// workgroup's staging copy of it is an L2 hit, not HBM traffic
static void format_bytes(DevMatrix& M, const std::vector<int4>& hh, const std::vector<int2>& blocks) {
    const int64_t n_rows = M.n_rows;
    const bool tiled = M.tiled;
    const int line_w = M.line_w;
    const int64_t xy = 8 * (M.n_cols_local + M.plan.n_halo()) + 8 * n_rows;
    int64_t fb = 2 * n_rows + xy, fb_tpl = xy;
    if (M.tpl.n > 0)
        fb_tpl += n_rows + 12 * (int64_t)M.tpl.n_ent + 12 * (int64_t)M.tpl.n;
    for (size_t q = 0; q < blocks.size(); ++q) {
        const int nz = hh[2 * q].w, nt = hh[2 * q + 1].y & 0xffff;
        const int64_t fb0 = fb;
        fb += 32;
        if (nz == 0) continue;
        if (nz > kCAP || (tiled && nt > kCAP / line_w)) {  // long row: CSR stream
            fb += 12 * (int64_t)nz;
            continue;
        }
        if (tiled) fb += 4 * (kCAP / line_w) + 2 * kCAP;  // tile ids, tile indices
        else if (M.col16.p) fb += 2 * (int64_t)nz + 16;   // column codes, band bases
        else fb += 4 * (int64_t)nz;                       // columns
        if (M.row_seg > 0) fb += 4 * (int64_t)(kTPB * M.gather_rpb / M.row_seg);  // segment rows the lanes load
        if (hh[2 * q + 1].z >= 0)
            fb += (tiled ? kCAP : gather_slots(nz) * kTPB) + 8 * (int64_t)hh[2 * q + 1].w;
        else
            fb += 8 * (int64_t)nz;
        if ((int)q >= M.nb_skip) fb_tpl += fb - fb0 + 2 * (int64_t)(blocks[q].y - blocks[q].x);
    }
    M.csr_fmt_bytes = fb;
    M.spmv_fmt_bytes = M.tpl.n > 0 ? fb_tpl : fb;
}

// Every device format from a CSR the caller keeps (H, never the member `host`):
// Solver::setup runs this on a worker thread while the hierarchy thread still reads the same
// CSR, and moves it into `host` after both are done.
// An operator's segment row map, checked before anything is uploaded: every segment lies
// inside the rows and every row belongs to exactly one (a bad map fails here, never in a kernel)
static void check_row_map(const std::vector<int>& seg_rows, int S, int64_t n_rows) {
    AMG_CHECK((S == 8 || S == 16 || S == 32) && n_rows % S == 0 && kTPB % S == 0, "row map: segment length");
    AMG_CHECK((int64_t)seg_rows.size() * S == n_rows, "row map: segment count");
    std::vector<char> seen((size_t)n_rows, 0);
    for (const int base : seg_rows) {
        AMG_CHECK(base >= 0 && (int64_t)base + S <= n_rows, "row map: segment outside the rows");
        for (int k = 0; k < S; ++k) {
            AMG_CHECK(!seen[(size_t)base + k], "row map: row covered twice");
            seen[(size_t)base + k] = 1;
        }
    }
}

// H's rows in the stored order of a segment row map (stored row i = vector row
// seg_rows[i / S] + i % S); columns, values and each row's entry order are H's
static HostCSR rows_in_stored_order(const HostCSR& H, const std::vector<int>& seg_rows, int S) {
    HostCSR B;
    B.n_global_rows = H.n_global_rows;
    B.n_global_cols = H.n_global_cols;
    B.row_starts = H.row_starts;
    B.col_starts = H.col_starts;
    const int64_t n = H.nrows();
    B.rp.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o = seg_rows[i / S] + i % S;
        B.rp[i + 1] = B.rp[i] + (H.rp[o + 1] - H.rp[o]);
    }
    B.col.resize((size_t)H.nnz());
    B.val.resize((size_t)H.nnz());
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < n / S; ++j) {  // a segment's rows are consecutive on both sides
        const int64_t o = seg_rows[j], k0 = H.rp[o], k1 = H.rp[o + S];
        std::copy(H.col.begin() + k0, H.col.begin() + k1, B.col.begin() + B.rp[j * S]);
        std::copy(H.val.begin() + k0, H.val.begin() + k1, B.val.begin() + B.rp[j * S]);
    }
    return B;
}

void DevMatrix::build_view(Context* c, const HostCSR& Hv, bool replicated_view) {
    // with a row map the formats are built from the rows in stored order; the caller's CSR
    // (vector order) stays the host image
    HostCSR stored;
    if (row_seg > 0) {
        AMG_CHECK(!replicated_view && blocks_only, "row map: a cycle copy only");
        check_row_map(seg_rows, row_seg, Hv.nrows());
        stored = rows_in_stored_order(Hv, seg_rows, row_seg);
    }
    const bool mapped = row_seg > 0;
    const HostCSR& H = mapped ? stored : Hv;
    seg.reset();
    prp.reset();
    ctx = c;
    replicated = replicated_view;
    static const HostComm serial;  // rank 0 of 1: replicated matrices have no halo
    const HostComm& comm = replicated ? serial : ctx->host;
    const BuildKnobs knobs = read_build_knobs();
    PhaseTimer tm(comm);
    AMG_CHECK((int)H.row_starts.size() == comm.nranks + 1, "matrix row partition size");
    AMG_CHECK((int)H.col_starts.size() == comm.nranks + 1, "matrix column partition size");
    first_row = H.row_starts[comm.rank];
    n_rows = H.nrows();
    AMG_CHECK(n_rows == H.row_starts[comm.rank + 1] - first_row, "local row count mismatch");
    first_col = H.col_starts[comm.rank];
    n_cols_local = H.col_starts[comm.rank + 1] - first_col;
    nnz = H.nnz();
    AMG_CHECK(nnz < INT_MAX && n_rows < INT_MAX, "local matrix exceeds int32 indexing");
    square = H.n_global_rows == H.n_global_cols && H.row_starts == H.col_starts;
    plan = halo_plan_for_cols(comm, H);
    if (send_map && !replicated)
        for (int64_t& v : plan.send_idx) v = (*send_map)[v];
    AMG_CHECK(n_cols_local + plan.n_halo() < INT_MAX, "too many columns for int32");
    tm.lap("    build: halo plan");

    std::vector<int> hrp;
    hvec<int> hcol;
    std::vector<uint8_t> cls;
    std::vector<double> di;
    TplBuild tb;
    std::vector<uint8_t> tplf;
    const std::vector<uint8_t>* tplf_p = nullptr;
    const bool dev_fmt = device_formats();
    CutChoice cut;
    BlockBuild bb;
    // the cut runs once; a second time, on the rows in vector order, only when it refuses a row map
    for (;;) {
        local_columns(H, plan, first_col, n_cols_local, hrp, hcol, cls);
        if (row_seg > 0) {  // a segment is cut as one: boundary class when any of its rows is
            for (int64_t j = 0; j < n_rows / row_seg; ++j) {
                uint8_t b = 0;
                for (int k = 0; k < row_seg; ++k) b |= cls[j * row_seg + k];
                for (int k = 0; k < row_seg; ++k) cls[j * row_seg + k] = b;
            }
        }
        rp.upload(hrp.data(), hrp.size());
        if (square) {
            std::vector<double> d = diagonal(comm, H);
            di.resize(n_rows);
#pragma omp parallel for schedule(static)
            for (int64_t i = 0; i < n_rows; ++i) di[i] = 1.0 / d[i];
            dinv.upload(di.data(), di.size());
        }
        tpl = TplFormat{};
        nb_skip = 0;
        if (square && n_rows > 0 && !blocks_only) tb = select_templates(knobs, H, hrp, hcol, di, n_cols_local);
        tm.lap("    build: local columns, dinv, templates");
        hcol.resize(nnz + kPad, 0);  // within the capacity local_columns reserved

        if (!tb.hdr.empty()) {
            tplf.resize(n_rows);
            for (int64_t i = 0; i < n_rows; ++i) tplf[i] = tb.id[i] != kTplNone && cls[i] == 0;
        }
        tplf_p = tplf.empty() ? nullptr : &tplf;
        // square operators: x tiles, one row per lane; short-row rectangular ones (gather
        // path): up to kGatherRPB rows per lane (profiles/r2n: P0 x += P e 162 -> 95 us; R
        // with 7+ entries per row was slower that way: R0 94 -> 106 us, sa27 R0 350 -> 415)
        gather_rpb = !square && nnz <= 4 * n_rows ? kGatherRPB : 1;
        const int unit = row_seg > 0 ? row_seg : 1;
        cut = choose_cut(knobs, hrp, hcol, cls, tplf_p, n_cols_local, plan.n_halo(), square, gather_rpb, unit);
        tiled = cut.tiled;
        tm.lap("    build: row blocks, sampled cuts");
        // The gather kernel reads x from global memory: its blocks need only the kCAP-entry and
        // row caps, not the 256-line tile cap.  sa27's R1 (270 entries per row over ~200 lines
        // each) was cut into blocks of ~1 row by that cap: one lane summing while 255 idled.
        const bool line_cap = tiled;
        bool map_ok = row_seg == 0 || (tiled && !square);
        if (map_ok) {
            bb = build_row_blocks(hrp, hcol, cls, n_cols_local, plan.n_halo(), tplf_p, kTPB * gather_rpb, line_cap,
                                  !dev_fmt, cut.line_w, 1, unit);
            // csr_block_rowmap_kernel has no long-row / empty-block path: every block must be a
            // tile block of whole segments
            for (size_t q = 0; map_ok && row_seg > 0 && q < bb.blocks.size(); ++q) {
                const int2 b = bb.blocks[q];
                const int nz = hrp[b.y] - hrp[b.x], nt = bb.tile_ptr[q + 1] - bb.tile_ptr[q];
                map_ok = nz > 0 && nz <= kCAP && nt > 0 && nt <= kCAP / cut.line_w && b.x % row_seg == 0 &&
                         b.y % row_seg == 0 && b.y - b.x <= kTPB * gather_rpb;
            }
        }
        if (map_ok) break;
        // refused: the operator is built as without a map, rows in vector order
        row_seg = 0;
        seg_rows.clear();
        stored = Hv;
    }
    line_w = cut.line_w;
    nb_int = bb.nb_int;
    nb_bnd = bb.nb_bnd;
    if (knobs.trace_blocks)
        std::fprintf(stderr, "[amg-blocks]   %s, lines of %d B: %zu blocks\n", tiled ? "x tile" : "gather",
                     8 * line_w, bb.blocks.size());
    tm.lap("    build: row blocks + x tiles");

    if (!tb.hdr.empty()) {
        nb_skip = bb.nb_skip;
        upload_templates(tpl, tb, bb, n_rows);
        const std::vector<int> ldo = tpl_window(tpl, tb);
        if (tpl.win > 0) {
            if (knobs.tpl_master) tpl.master = find_master_template(tb, ldo);
            tpl_march(tpl, n_rows);
        }
    }
    tm.lap("    build: template window / march");

    blocks.upload(bb.blocks.data(), bb.blocks.size());
    const size_t nbk = bb.blocks.size();
    // device col / val: block-aligned copies -- block q's entries at an even offset
    // koff[q] (16-byte aligned values), so the kernel reads them as (2t, 2t + 1) pairs
    std::vector<int64_t> koff(nbk + 1, 0);
    for (size_t q = 0; q < nbk; ++q)
        koff[q + 1] = koff[q] + (int64_t)(hrp[bb.blocks[q].y] - hrp[bb.blocks[q].x] + 1) / 2 * 2;
    AMG_CHECK(koff[nbk] + kPad < INT_MAX, "local matrix exceeds int32 indexing");
    FormatHeaderInfo fi;
    if (dev_fmt) {
        // per-nonzero streams built on the GPU from one upload of the CSR (formats.hip)
        build_formats_device(*this, hrp, hcol, H.val, bb.blocks, bb.tile_ptr, bb.tile_lines, koff, fi);
        tm.lap("    build: device col / val / tiles / value index / row ends");
    } else {
        host_block_streams(*this, tm, H, hrp, hcol, bb, koff, fi);
    }
    col16.reset();
    gband.reset();
    if (!tiled && nbk > 0) gather_codes(hrp, hcol, bb.blocks, koff, col16, gband);
    const std::vector<int4> hh = block_headers(*this, hrp, bb, koff, fi);
    hdr.upload(hh.data(), hh.size());
    if (row_seg > 0) upload_block_segments(*this, bb.blocks);
    // measured (profiles/r1m_variants.txt): x tiles in XCD order on square operators (A0
    // -6..8%, A1 -6..8%, A2 +1% vs plain order; gathers are 1.3-1.9x slower); gathers in
    // XCD order on the rectangular P / R (R0 -10% vs plain order)
    default_variant = tiled ? KV_XCD : (KV_GATHER | KV_XCD);
    format_bytes(*this, hh, bb.blocks);
    tm.lap("    build: row ends, headers");

    std::vector<int> sidx(plan.send_idx.begin(), plan.send_idx.end());
    send_idx.upload(sidx.data(), sidx.size());
    send_buf.alloc(sidx.size());
    halo.alloc(plan.n_halo());
    // collective order: the same id on every rank.  Only the loopback transport matches
    // matrices by it, and only one rank's setup builds formats on worker threads (several at
    // once), so the counter is touched where it is used
    if (ctx->transport == TR_LOOPBACK && !replicated) {
        seq = ctx->mat_seq++;
        loopback_register(*ctx, seq, send_buf.p, plan.send_procs, plan.send_ptr);
    }
}

// The GS chunks of an operator's local rows (global multiples of B clipped to the rank) and
// the in-chunk new-value couplings of a sweep in direction d (0 forward, 1 backward): row i
// (local ids) with global column gc, forward cs <= j < i, backward i < j < ce
// (hybrid_gs_kernel's [lo, hi))
struct GsChunks {
    int64_t first_row, n_rows, clo, chi, B;
    explicit GsChunks(const DevMatrix& M)
        : first_row(M.first_row), n_rows(M.n_rows), clo(M.first_col), chi(M.first_col + M.n_cols_local),
          B(M.gs.block) {}
    bool is_new(int d, int64_t i, int64_t gc) const {
        if (gc < clo || gc >= chi) return false;
        const int64_t j = gc - clo, g = first_row + i;
        const int64_t cs = std::max<int64_t>(0, (g / B) * B - first_row);
        const int64_t ce = std::min<int64_t>(n_rows, (g / B + 1) * B - first_row);
        return d == 0 ? (j >= cs && j < i) : (j > i && j < ce);
    }
};

// The split sweep's old-value pass for direction d (0 forward, 1 backward): this operator
// without the sweep's in-chunk new-value couplings, as a CSR-block matrix of its own (4.2c).
// Collective on N ranks (its halo plan); never inside a graph capture (Solver::setup builds
// what the cycle needs).
void DevMatrix::ensure_gs_pass(int d) {
    if (gs.split.old[d]) return;
    const HostCSR& H = host_image();  // the member `host`, or the CSR a worker builds from
    AMG_CHECK(gs.split.on && gs.block > 0, "hybrid GS: no split sweep for this operator");
    AMG_CHECK(!ctx->capturing, "hybrid GS: split pass requested inside a graph capture");
    const GsChunks ch(*this);
    HostCSR h;
    h.n_global_rows = H.n_global_rows;
    h.n_global_cols = H.n_global_cols;
    h.row_starts = H.row_starts;
    h.col_starts = H.col_starts;
    h.rp.assign((size_t)n_rows + 1, 0);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; ++i) {
        int64_t c = 0;
        for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k) c += !ch.is_new(d, i, H.col[k]);
        h.rp[i + 1] = c;
    }
    for (int64_t i = 0; i < n_rows; ++i) h.rp[i + 1] += h.rp[i];
    h.col.resize((size_t)h.rp[n_rows]);
    h.val.resize((size_t)h.rp[n_rows]);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; ++i) {
        int64_t o = h.rp[i];
        for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k)
            if (!ch.is_new(d, i, H.col[k])) {
                h.col[o] = H.col[k];
                h.val[o] = H.val[k];
                ++o;
            }
    }
    // CSR blocks only: no row templates (and so no windows, masks or march tables) are built
    // for the pass's operator, and its format is set before the build -- no
    // format_generation bump, no captured graph goes stale
    gs.split.old[d] = std::make_unique<DevMatrix>();
    gs.split.old[d]->blocks_only = true;
    gs.split.old[d]->format = AMG_FORMAT_BLOCKS;
    gs.split.old[d]->build(ctx, std::move(h), replicated);
}

// The one-kernel sweep's sliced ELL (hybrid_gs_kernel): every entry of the ELL slabs, with a
// value dictionary when the local operator takes <= 256 distinct values.  Built with the GS
// blocks unless the operator runs split sweeps (4.2c), whose passes never read it; then on
// first use (a norm-carrying forward sweep: Solver::setup builds it for level 0).  r5: sa27's
// level-1 / level-2 GS builds spent ~1.9 s of an 8.1 s setup mostly here.
void DevMatrix::ensure_gs_ell() {
    if (gs.ell_built) return;
    const HostCSR& H = host_image();  // the member `host`, or the CSR a worker builds from
    AMG_CHECK(!ctx->capturing, "hybrid GS: sliced ELL requested inside a graph capture");
    const int64_t clo = first_col, chi = first_col + n_cols_local;
    auto local_col = [&](int64_t g) -> int {
        return g >= clo && g < chi ? (int)(g - clo) : (int)(n_cols_local + plan.find(g));
    };
    const std::vector<int4>& slabs = gs.slabs_host;
    const int64_t cells = gs.cells;
    std::vector<int> sc((size_t)(cells + 4) * 64, -1);
    std::vector<double> sv(sc.size(), 0.0);
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t q = 0; q < slabs.size(); ++q) {
        const int4 sl = slabs[q];
        for (int l = 0; l < sl.y; ++l) {
            const int64_t i = sl.x + l;
            for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k) {
                const size_t at = ((size_t)sl.z + (size_t)(k - H.rp[i])) * 64 + l;
                sc[at] = local_col(H.col[k]);
                sv[at] = H.val[k];
            }
        }
    }
    // value dictionary: <= 256 distinct values (bit patterns) in the local operator; each
    // thread scans a chunk into a small set and gives up past 256
    std::vector<uint64_t> dict;
    {
        const int64_t nz = (int64_t)H.val.size();
        std::atomic<bool> over{false};
#pragma omp parallel
        {
            std::vector<uint64_t> mine;
#pragma omp for schedule(static) nowait
            for (int64_t k = 0; k < nz; ++k) {
                if (over.load(std::memory_order_relaxed)) continue;
                uint64_t bits;
                std::memcpy(&bits, &H.val[k], sizeof(bits));
                if (std::find(mine.begin(), mine.end(), bits) == mine.end()) {
                    mine.push_back(bits);
                    if (mine.size() > 256) over.store(true, std::memory_order_relaxed);
                }
            }
#pragma omp critical
            if (!over.load()) dict.insert(dict.end(), mine.begin(), mine.end());
        }
        std::sort(dict.begin(), dict.end());
        dict.erase(std::unique(dict.begin(), dict.end()), dict.end());
        if (over.load() || dict.size() > 256) dict.clear();
    }
    gs.ndict = (int)dict.size();
    if (gs.ndict > 0) {
        std::vector<uint8_t> vid(sc.size(), 0);
#pragma omp parallel for schedule(dynamic, 64)
        for (size_t q = 0; q < slabs.size(); ++q) {
            const int4 sl = slabs[q];
            for (int l = 0; l < sl.y; ++l)
                for (int k = 0; k < sl.w; ++k) {
                    const size_t at = ((size_t)sl.z + (size_t)k) * 64 + (size_t)l;
                    if (sc[at] < 0) continue;
                    uint64_t bits;
                    std::memcpy(&bits, &sv[at], sizeof(bits));
                    vid[((size_t)sl.z + (size_t)(k & ~3)) * 64 + 4 * (size_t)l + (size_t)(k & 3)] =
                        (uint8_t)(std::lower_bound(dict.begin(), dict.end(), bits) - dict.begin());
                }
        }
        std::vector<double> tab(dict.size());
        std::memcpy(tab.data(), dict.data(), sizeof(double) * dict.size());
        gs.vid.upload(vid.data(), vid.size());
        gs.vtab.upload(tab.data(), tab.size());
        gs.val.reset();
    } else {
        gs.vid.reset();
        gs.vtab.reset();
        gs.val.upload(sv.data(), sv.size());
    }
    gs.col.upload(sc.data(), sc.size());
    gs.ell_built = true;
}

// ---- the stages of DevMatrix::ensure_gs_blocks, in the order it runs them.  H is the
// operator's host image.

// l1 diagonal of every row: 1 / d_i, d_i = a_ii + sum of |a_ij| outside the row's chunk (global
// multiples of B clipped to the rank), summed in CSR order like the oracle
static std::vector<double> gs_l1_diagonal(const HostCSR& H, int64_t first_row, int64_t B) {
    const int64_t n_rows = H.nrows();
    std::vector<double> di(n_rows);
    std::atomic<bool> zero_row{false};
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t g = first_row + i;
        const int64_t cs = std::max<int64_t>(first_row, g / B * B);
        const int64_t ce = std::min(first_row + n_rows, (g / B + 1) * B);
        double l1 = 0.0, d = 0.0;
        for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k) {
            const int64_t gc = H.col[k];
            if (gc < cs || gc >= ce) l1 += std::fabs(H.val[k]);
            if (gc == g) d = H.val[k];
        }
        if (d == 0.0 && l1 == 0.0) zero_row.store(true, std::memory_order_relaxed);
        di[i] = 1.0 / (d + l1);
    }
    AMG_CHECK(!zero_row.load(), "hybrid GS: zero row");
    return di;
}

// GS templates: a 512-row block runs on tpl_gs_kernel when every row has
// a row template (all columns local) and the (template, l1 diagonal) pairs fit the table.
// Chunks must not straddle a wave's 64-row group: first_row % 64 == 0 and B | 64.
// Fills G from the row templates' host table; returns per 512-row block 1 = on the template
// kernel (empty: none is).
static std::vector<char> gs_templates(GsFormat::Tpl& G, const TplFormat& T, const std::vector<double>& di,
                                      int64_t first_row, int64_t B) {
    const int64_t n_rows = (int64_t)di.size();
    // the template kernels take one chain coupling per row: every template's in-chunk
    // offsets (0 < |o| < B) must be -1 / +1 only
    bool shape_ok = T.n > 0 && T.win > 0;
    for (int o : T.off_host)
        if (o != 0 && o != -1 && o != 1 && std::llabs(o) < B) shape_ok = false;
    if (!shape_ok || first_row % 64 != 0 || 64 % B != 0 || (int64_t)T.id_host.size() != n_rows) return {};
    std::vector<uint8_t> gid((size_t)n_rows, (uint8_t)kTplNone);
    std::vector<std::vector<std::pair<uint64_t, int>>> by_tpl(T.n);
    std::vector<int> gbase;
    std::vector<double> gdl;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int t = T.id_host[i];
        if (t == kTplNone) continue;
        uint64_t bits;
        std::memcpy(&bits, &di[i], sizeof(bits));
        int found = -1;
        for (const auto& pr : by_tpl[t])
            if (pr.first == bits) {
                found = pr.second;
                break;
            }
        if (found < 0) {
            if ((int)gbase.size() >= kTplMax) return {};
            found = (int)gbase.size();
            gbase.push_back(t);
            gdl.push_back(di[i]);
            by_tpl[t].push_back({bits, found});
        }
        gid[i] = (uint8_t)found;
    }
    const int64_t nb = (n_rows + kTplRows - 1) / kTplRows;
    std::vector<char> tblk((size_t)nb, 0);
    std::vector<int> blist;
    for (int64_t q = 0; q < nb; ++q) {
        bool all = true;
        for (int64_t i = q * kTplRows; i < std::min(n_rows, (q + 1) * kTplRows) && all; ++i)
            all = gid[i] != kTplNone;
        if (all) {
            tblk[q] = 1;
            blist.push_back((int)q);
        }
    }
    if (blist.empty()) return {};
    std::vector<int> gh(gbase.size()), cf(gbase.size(), 0);
    std::vector<int> kem(gbase.size(), -1), kep(gbase.size(), -1);
    std::vector<double> cvm(gbase.size(), 0.0), cvp(gbase.size(), 0.0);
    for (size_t k = 0; k < gbase.size(); ++k) {
        const int h = T.hdr_host[gbase[k]];
        gh[k] = h;
        const int st = h & 0xffff, ln = (h >> 16) & 0xff;
        for (int e = st; e < st + ln; ++e) {
            if (T.off_host[e] == -1) cvm[k] = T.val_host[e], cf[k] |= 1, kem[k] = e - st;
            if (T.off_host[e] == 1) cvp[k] = T.val_host[e], cf[k] |= 2, kep[k] = e - st;
        }
    }
    G.cvm.upload(cvm.data(), cvm.size());
    G.cvp.upload(cvp.data(), cvp.size());
    G.cf.upload(cf.data(), cf.size());
    G.kem.upload(kem.data(), kem.size());
    G.kep.upload(kep.data(), kep.size());
    G.racc.alloc((size_t)n_rows);
    G.id.upload(gid.data(), gid.size());
    G.hdr.upload(gh.data(), gh.size());
    G.dl.upload(gdl.data(), gdl.size());
    G.blocks.upload(blist.data(), blist.size());
    if (T.master.ne > 0) {  // uniform stencil: a GS template's mask is its row template's
        std::vector<unsigned> gm(gbase.size());
        for (size_t k = 0; k < gbase.size(); ++k) gm[k] = T.master.mask_host[gbase[k]];
        G.mask.upload(gm.data(), gm.size());
    }
    G.n = (int)gbase.size();
    G.n_blk = (int)blist.size();
    return tblk;
}

// The rows off the template kernel: chunks packed whole into <= 64-row slabs; interior slabs
// (no halo column) first, so par_hybrid_gs runs them while the halo is in flight.  Returns the
// slabs {first row, rows, offset / 64, width} in that order, their count of interior slabs and
// of sliced-ELL cells.
static std::vector<int4> gs_pack_slabs(const HostCSR& H, const std::vector<char>& tblk, int64_t first_row,
                                       int64_t first_col, int64_t n_cols_local, int64_t B, int& n_int,
                                       int64_t& cells) {
    const int64_t n_rows = H.nrows();
    auto on_tpl = [&](int64_t r) { return !tblk.empty() && tblk[(size_t)(r / kTplRows)] != 0; };
    std::vector<int4> slabs;
    std::vector<char> sbnd;
    for (int64_t r = 0; r < n_rows;) {
        if (on_tpl(r)) {
            r = std::min(n_rows, (r / kTplRows + 1) * kTplRows);
            continue;
        }
        int64_t end = r;
        while (end < n_rows && !on_tpl(end)) {
            const int64_t g = first_row + end;
            const int64_t ce = std::min(n_rows, (g / B + 1) * B - first_row);
            if (ce - r > 64) break;
            end = ce;
        }
        AMG_ASSERT(end > r);
        int w = 0;
        char bnd = 0;
        for (int64_t i = r; i < end; ++i) {
            w = std::max<int>(w, (int)(H.rp[i + 1] - H.rp[i]));
            for (int64_t k = H.rp[i]; k < H.rp[i + 1] && !bnd; ++k)
                bnd = H.col[k] < first_col || H.col[k] >= first_col + n_cols_local;
        }
        slabs.push_back(make_int4((int)r, (int)(end - r), 0, w));
        sbnd.push_back(bnd);
        r = end;
    }
    std::vector<int4> ordered;
    ordered.reserve(slabs.size());
    for (int pass = 0; pass < 2; ++pass)
        for (size_t q = 0; q < slabs.size(); ++q)
            if (sbnd[q] == pass) ordered.push_back(slabs[q]);
    n_int = 0;
    for (char c : sbnd) n_int += c == 0;
    cells = 0;
    for (int4& sl : ordered) {
        sl.z = (int)cells;
        cells += (sl.w + 3) & ~3;  // slabs start at multiples of 4 cells (dictionary dwords)
    }
    AMG_CHECK((cells + 4) * 64 < INT_MAX, "hybrid GS: sliced-ELL too large for int32 offsets");
    return ordered;
}

// The chain ELL of direction d: the same slabs, only the new-value couplings, in consumption
// order.  Fills S's arrays of direction d; returns the ELL's cells.
static int64_t gs_chain_ell(GsFormat::Split& S, int d, const HostCSR& H, const GsChunks& ch,
                            const std::vector<int4>& slabs) {
    std::vector<int4> cs = slabs;
    int64_t cc = 0;
    for (int4& sl : cs) {
        int w = 0;
        for (int l = 0; l < sl.y; ++l) {
            const int64_t i = sl.x + l;
            int c = 0;
            for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k) c += ch.is_new(d, i, H.col[k]);
            w = std::max(w, c);
        }
        sl.z = (int)cc;
        sl.w = w;
        cc += (w + 3) & ~3;
    }
    std::vector<int> ccol((size_t)(cc + 4) * 64, -1);
    std::vector<double> cval(ccol.size(), 0.0);
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t q = 0; q < cs.size(); ++q) {
        const int4 sl = cs[q];
        for (int l = 0; l < sl.y; ++l) {
            const int64_t i = sl.x + l;
            int c = 0;
            // consumption order: forward ascending, backward descending column
            for (int64_t kk = H.rp[i]; kk < H.rp[i + 1]; ++kk) {
                const int64_t k = d == 0 ? kk : H.rp[i + 1] - 1 - (kk - H.rp[i]);
                if (ch.is_new(d, i, H.col[k])) {
                    const size_t at = ((size_t)sl.z + (size_t)c++) * 64 + l;
                    ccol[at] = (int)(H.col[k] - ch.clo);
                    cval[at] = H.val[k];
                }
            }
        }
    }
    // one chain launch: every slab in the widest slab's width bucket (one launch per
    // bucket measured slower, g3sub 1560 -> 1360 V-cycles/s: the coarse levels pay
    // the extra launches, profiles/r4f_g3sub_buckets.txt)
    int wmax = 0;
    for (const int4& sl : cs) wmax = std::max(wmax, sl.w);
    for (int q = 0; q <= kGsChainBuckets; ++q) S.cbucket[d][q] = 0;
    S.cbucket[d][gs_chain_bucket(wmax) + 1] = (int)cs.size();
    for (int q = 0; q < kGsChainBuckets; ++q) S.cbucket[d][q + 1] += S.cbucket[d][q];
    S.cslabs[d].upload(cs.data(), cs.size());
    S.ccol[d].upload(ccol.data(), ccol.size());
    S.cval[d].upload(cval.data(), cval.size());
    S.cmaxw[d] = wmax;
    return cc;
}

void DevMatrix::ensure_gs_blocks(int64_t B) {
    const HostCSR& H = host_image();  // the member `host`, or the CSR a worker builds from
    AMG_CHECK(square, "hybrid GS needs a square matrix");
    AMG_CHECK(B >= 1 && B <= 64, "hybrid GS block must be in [1, 64]");
    if (gs.block == B) return;
    const BuildKnobs knobs = read_build_knobs();
    gs = GsFormat{};  // a build for another block size starts from nothing
    const std::vector<double> di = gs_l1_diagonal(H, first_row, B);
    std::vector<char> tblk;
    if (knobs.gs_templates) tblk = gs_templates(gs.tpl, tpl, di, first_row, B);
    std::vector<int4> slabs = gs_pack_slabs(H, tblk, first_row, first_col, n_cols_local, B, gs.n_slabs_int, gs.cells);
    const int64_t cells = gs.cells;
    gs.slabs.upload(slabs.data(), slabs.size());
    gs.dinv.upload(di.data(), di.size());
    gs.n_slabs = (int)slabs.size();
    gs.block = B;
    // bytes per sweep: ELL cells + slab headers + 32 B per ELL row (b, x, dinv, y)
    int64_t ell_rows = 0;
    for (const int4& sl : slabs) ell_rows += sl.y;
    gs.bytes = (gs.ndict > 0 ? 5 : 12) * 64 * cells + 16 * (int64_t)slabs.size() + 32 * ell_rows;
    // template rows: acc kernel 1 B id + b + x (window) + acc out; chain kernel acc + x + id + y
    if (gs.tpl.n_blk > 0)
        gs.bytes += 50 * (n_rows - ell_rows) + 16 * (int64_t)tpl.n_ent + 12 * (int64_t)gs.tpl.n;
    gs.wide = !slabs.empty() && cells >= (int64_t)kGsWide * (int64_t)slabs.size();

    // Split sweeps: the old-value couplings as a CSR-block pass (KM_GSACC on A
    // without the sweep's in-chunk new-value couplings -- the same entries in the same order,
    // so acc is bit-identical) and the chain walk on a sliced ELL of the new-value couplings
    // only.  No GS template rows, and rows of >= AMG_GS_SPLIT_NPR entries on average (default
    // 12: g3sub's 5.5-entry level 0 ran 60 -> 72 us per sweep split, its 45-entry level 1
    // 121 -> 63 us; profiles/r3u_split_ab.txt; 0 forces it, tests).  On N ranks (r5) the pass
    // is a distributed matrix of its own: its off-rank columns are A's (chunks never cross a
    // rank cut, so every in-chunk coupling is local), par_apply exchanges their halo while the
    // interior blocks run, and the old values across ranks are the Jacobi-across-ranks half of
    // the oracle's rank-cut definition -- results unchanged.  The pass is built collectively,
    // so the ranks agree first: all split or none do.
    bool split = knobs.gs_split && gs.tpl.n_blk == 0 && n_rows > 0 && nnz >= knobs.gs_split_npr * n_rows;
    if (ctx->host.nranks > 1 && !replicated)
        for (int64_t v : ctx->host.allgather((int64_t)(split ? 1 : 0))) split = split && v != 0;
    gs.slabs_host = slabs;
    if (!split) {
        ensure_gs_ell();
        return;
    }
    gs.split.on = true;  // (ensure_gs_pass checks it)
    // the backward pass (post-smoothing) is built now; the forward one on first use
    // (ensure_gs_pass): a coarse level's forward sweep starts from x = 0 and skips it
    // (par_hybrid_gs_from_zero)
    const GsChunks ch(*this);
    const int64_t ccells = gs_chain_ell(gs.split, 0, H, ch, slabs);
    ensure_gs_pass(1);
    gs_chain_ell(gs.split, 1, H, ch, slabs);
    gs.split.acc.alloc((size_t)n_rows);
    // bytes per (forward) sweep: the pass (its stored format + b + acc out), then the
    // chain ELL cells + slab headers + acc, x, dinv in and y out
    gs.bytes = gs.split.old[1]->mode_bytes(KM_RESID) + 8 * n_rows + 12 * 64 * ccells +
               16 * (int64_t)slabs.size() + 32 * n_rows;
}

int64_t DevMatrix::format_generation = 0;

int64_t DevMatrix::mode_bytes(int mode) const {
    const int64_t n = n_rows;
    if (format == AMG_FORMAT_CSR) {  // residual + 8 n (b), Jacobi + 16 n (b, dinv)
        const int64_t base = csr_plain_bytes();
        return base + (mode == KM_CHEBY ? 24 * n : mode == KM_JACOBI ? 16 * n : mode == KM_SPMV ? 0 : 8 * n);
    }
    const bool tpl = tpl_on();
    int64_t b = tpl ? spmv_fmt_bytes : csr_fmt_bytes;
    if (mode != KM_SPMV) b += 8 * n;  // b, or y for y += A x
    // template rows take 1/a_ii and x[r] from LDS; CSR-kernel rows stream them
    if (mode == KM_JACOBI || mode == KM_CHEBY) b += tpl ? jac_extra_csr : jac_extra_all;
    if (mode == KM_CHEBY) b += 8 * n;  // Jacobi + xprev
    return b;
}

void DevMatrix::set_format(int f) {
    AMG_CHECK(f == AMG_FORMAT_AUTO || f == AMG_FORMAT_CSR || f == AMG_FORMAT_BLOCKS, "bad format");
    if (f == AMG_FORMAT_CSR && !pcol.p && nnz + 2 > 0) {
        // plain arrays in local | halo numbering, in row order (row_ptr is `rp`); two padding
        // entries (column 0, value 0) keep the kernel's last 16-byte pair inside the buffer
        const int64_t clo = first_col, chi = first_col + n_cols_local;
        std::vector<int> pc((size_t)nnz + 2, 0);
        std::vector<double> pv((size_t)nnz + 2, 0.0);
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < nnz; ++k) {
            const int64_t g = host.col[k];
            pc[k] = g >= clo && g < chi ? (int)(g - clo) : (int)(n_cols_local + plan.find(g));
            pv[k] = host.val[k];
        }
        pcol.upload(pc.data(), pc.size());
        pval.upload(pv.data(), pv.size());
        if (row_seg > 0) {  // `rp` follows the stored rows; the plain kernel walks the vector's
            std::vector<int> pr(host.rp.begin(), host.rp.end());
            prp.upload(pr.data(), pr.size());
        }
    }
    if (f != AMG_FORMAT_CSR) {
        // the plain arrays (12 B per nonzero) are rebuilt when CSR is selected again; hipFree
        // waits for the kernels that may still read them
        pcol.reset();
        pval.reset();
        prp.reset();
    }
    if (format != f) ++format_generation;
    format = f;
}

bool DevMatrix::halo_begin(const double* x) {
    const HostComm& comm = ctx->host;
    if (comm.nranks == 1 || replicated) return false;
    hipStream_t s = ctx->stream, cs = ctx->comm_stream;
    if (ctx->transport == TR_LOOPBACK) {  // collective on every rank, even with no neighbours
        loopback_before_pack(*ctx, plan.send_procs);
        launch_pack(s, (int64_t)plan.send_idx.size(), send_idx.p, x, send_buf.p);
        loopback_halo(*ctx, seq, send_buf.p, halo.p, plan.send_procs, plan.recv_procs,
                      plan.recv_ptr, true);
        return true;
    }
    if (plan.send_idx.empty() && plan.halo_gid.empty()) return false;
    ctx->eager_rccl_fence();
    static const bool trace = std::getenv("AMG_TRACE_RCCL") != nullptr;
    if (trace) std::fprintf(stderr, "[amg] rank %d halo_begin seq %lld send %zu recv %lld\n", comm.rank,
                            (long long)seq, plan.send_idx.size(), (long long)plan.n_halo());
    launch_pack(s, (int64_t)plan.send_idx.size(), send_idx.p, x, send_buf.p);
    HIP_CHECK(hipEventRecord(ctx->ev_pack, s));
    HIP_CHECK(hipStreamWaitEvent(cs, ctx->ev_pack, 0));
    NCCL_CHECK(ncclGroupStart());
    for (size_t p = 0; p < plan.send_procs.size(); ++p)
        NCCL_CHECK(ncclSend(send_buf.p + plan.send_ptr[p], (size_t)(plan.send_ptr[p + 1] - plan.send_ptr[p]),
                            ncclDouble, plan.send_procs[p], ctx->nccl, cs));
    for (size_t p = 0; p < plan.recv_procs.size(); ++p)
        NCCL_CHECK(ncclRecv(halo.p + plan.recv_ptr[p], (size_t)(plan.recv_ptr[p + 1] - plan.recv_ptr[p]),
                            ncclDouble, plan.recv_procs[p], ctx->nccl, cs));
    NCCL_CHECK(ncclGroupEnd());
    if (trace) std::fprintf(stderr, "[amg] rank %d halo group enqueued\n", comm.rank);
    HIP_CHECK(hipEventRecord(ctx->ev_halo, cs));
    return true;
}

void DevMatrix::halo_wait() { HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0)); }

void par_apply(DevMatrix& A, int mode, const double* x, const double* b, double* y, double omega,
               double* partial, const double* xprev, double c1) {
    if (mode == KM_JACOBI || mode == KM_RESID || mode == KM_CHEBY)
        AMG_CHECK(A.square, "Jacobi/residual need a square matrix");
    const bool comm = A.halo_begin(x);
    hipStream_t s = A.ctx->stream;
    const bool norm = partial != nullptr;
    if (A.format == AMG_FORMAT_CSR) {  // plain CSR: one launch over every row, after the halo
        if (comm) A.halo_wait();
        launch_csr_plain(s, mode, norm, A, x, b, y, omega, partial, xprev, c1);
        return;
    }
    // template rows never touch the halo: they run with the interior blocks; the CSR kernel's
    // partials follow the template kernel's
    const bool tp = A.tpl_on();
    const int c0 = tp ? A.nb_skip : 0;
    const int poff = tp ? (A.tpl.blocks(A.n_rows) - A.nb_skip) * kNormParts : 0;
    if (tp) launch_tpl(s, mode, norm, A, x, b, y, omega, partial, xprev, c1);
    launch_csr_stream(s, mode, norm, A, c0, A.nb_int - c0, x, b, y, omega, partial, poff, nullptr, nullptr, xprev, c1);
    if (comm) A.halo_wait();
    launch_csr_stream(s, mode, norm, A, A.nb_int, A.nb_bnd, x, b, y, omega, partial, poff, nullptr, nullptr, xprev, c1);
}

bool par_restrict_j0(DevMatrix& R, const double* r, double* bc, double* x0c, const double* dinvc,
                     double omega) {
    if (R.format == AMG_FORMAT_CSR || R.tpl_on()) return false;
    const bool comm = R.halo_begin(r);
    hipStream_t s = R.ctx->stream;
    launch_csr_stream(s, KM_SPMV, false, R, 0, R.nb_int, r, nullptr, bc, omega, nullptr, 0, x0c, dinvc);
    if (comm) R.halo_wait();
    launch_csr_stream(s, KM_SPMV, false, R, R.nb_int, R.nb_bnd, r, nullptr, bc, omega, nullptr, 0, x0c, dinvc);
    return true;
}

void par_hybrid_gs(DevMatrix& A, const double* x, const double* b, double* y, int64_t block,
                   bool backward, double* partial) {
    A.ensure_gs_blocks(block);
    if (A.gs.split.on && !partial) {  // split sweep: the pass exchanges its halo
        A.ensure_gs_pass(backward ? 1 : 0);
        par_apply(*A.gs.split.old[backward ? 1 : 0], KM_GSACC, x, b, A.gs.split.acc.p, 0.0, nullptr);
        launch_gs_chain(A.ctx->stream, A, x, A.gs.split.acc.p, y, backward);
        return;
    }
    A.ensure_gs_ell();
    const bool comm = A.halo_begin(x);
    hipStream_t s = A.ctx->stream;
    // template blocks and interior slabs never read the halo: they run while it is in flight
    launch_hybrid_gs(s, A, x, b, y, backward, partial, 0, A.gs.n_slabs_int, true);
    if (comm) A.halo_wait();
    launch_hybrid_gs(s, A, x, b, y, backward, partial, A.gs.n_slabs_int, A.gs.n_slabs, false);
}

// Forward sweep from x = 0 (the first pre-smoothing sweep of a coarse level): every old-value
// term is a_ij * 0.0 = +-0.0, so acc = b bit for bit (b - (+-0.0) == b, and where b is -0.0
// the new x_i = 0.0 + acc * d is +0.0 either way) -- the split sweep's old-value pass and its
// halo exchange are skipped and the chain walk starts from acc = b.  Other forms sweep as usual.
void par_hybrid_gs_from_zero(DevMatrix& A, const double* x0, const double* b, double* y, int64_t block) {
    A.ensure_gs_blocks(block);
    if (A.gs.split.on) {
        launch_gs_chain(A.ctx->stream, A, x0, b, y, false);
        return;
    }
    par_hybrid_gs(A, x0, b, y, block, false);
}

void norm_finish(DevMatrix& A, const NormSink& ns, int nparts) {
    Context* c = A.ctx;
    const int nb = nparts >= 0 ? nparts : A.norm_parts();
    const int nr = c->host.nranks;
    double* local = ns.gathered + nr;
    // one rank: the reduction and the finish in one launch
    if (nr == 1 && launch_reduce_norm(c->stream, nb, ns.partial, ns.tmp, ns.done, local, ns.hist, ns.counter))
        return;
    if (nb > 0) launch_reduce_partials(c->stream, nb, ns.partial, ns.tmp, local);
    else launch_zero(c->stream, 1, local);
    if (nr > 1) {
        c->allgather(local, ns.gathered, 1);
        launch_finish_norm(c->stream, nr, ns.gathered, ns.hist, ns.counter);
    } else {
        launch_finish_norm(c->stream, 1, local, ns.hist, ns.counter);
    }
}

void par_residual_norm(DevMatrix& A, const double* x, const double* b, double* r,
                       const NormSink& ns) {
    par_apply(A, KM_RESID, x, b, r, 0.0, ns.partial);
    norm_finish(A, ns);
}

}  // namespace amg
