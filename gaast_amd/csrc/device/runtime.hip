// C ABI of the gfx950 back end (include/gaast_hip.h): device storage of graded rows, program
// objects (launch plans) and the batched evaluator.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../common/metric_basis.hpp"
#include "comm.hpp"
#include "gaast_expr.h"
#include "gaast_hip.h"
#include "jit_cache.hpp"
#include "kernels.hip.hpp"
#include "plan.hpp"

using namespace gaast;

// revision of everything that decides which kernel code runs (csrc/Makefile: KREV)
#ifndef GAAST_KERNELS_REV
#define GAAST_KERNELS_REV "unknown"
#endif

// ------------------------------------------------------------------------------------------
// state
// ------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_err;
bool g_init = false;
int g_device = -1;
hipStream_t g_stream = nullptr;
int g_num_cu = 256;
size_t g_max_lds = 160 * 1024;
Comm g_comm;                       // the gather communicator (gaast_hip_comm_init), if any
std::vector<hipEvent_t> g_events;  // chunk-done events of gaast_hip_eval_gather, created on demand
hipEvent_t g_comm_done = nullptr;
int64_t* g_comm_flag = nullptr;    // device word of gaast_hip_eval_gather's collective error flag
// partial rows of gaast_hip_mv_sum_rows, one buffer per stream it ran on (reductions on two streams never share one); grown on
// demand after a synchronisation of that stream only, freed at shutdown
struct ReduceScratch {
    hipStream_t stream;
    void* ptr;
    size_t bytes;
};
std::vector<ReduceScratch> g_reduce_scratch;

int set_err(int status, const std::string& msg) {
    g_err = msg;
    return status;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return set_err(GAAST_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// Every entry point that touches the GPU starts here: HIP's current device is per host thread, the library's
// device is per process (include/gaast_hip.h, conventions).
int ensure_init() {
    if (!g_init) return set_err(GAAST_ERR_NO_DEVICE, "gaast_hip_init() has not been called (or found no GPU)");
    HIP_TRY(hipSetDevice(g_device));
    return GAAST_OK;
}

size_t dtype_size(int dtype) { return dtype == GAAST_F32 ? 4 : 8; }

// internal status of program creation: a chained step went beyond the LDS the plan builder had budgeted (reported as
// GAAST_ERR_UNIMPLEMENTED once gaast_hip_program_create has tried the program without chains)
constexpr int kChainTooBig = -1000;

// One device allocation of `count` elements, freed with its owner
struct DevTable {
    void* ptr = nullptr;
    size_t count = 0;
    DevTable() = default;
    DevTable(DevTable&& o) noexcept : ptr(o.ptr), count(o.count) {
        o.ptr = nullptr;
        o.count = 0;
    }
    DevTable& operator=(DevTable&& o) noexcept {
        std::swap(ptr, o.ptr);
        std::swap(count, o.count);
        return *this;
    }
    ~DevTable() {
        if (ptr) (void)hipFree(ptr);
    }
    template <typename T>
    const T* as() const { return static_cast<const T*>(ptr); }
    // an index table, as it is (the host image goes with the argument)
    template <typename I>
    int upload(std::vector<I> v) {
        return upload_bytes(v.data(), v.size(), sizeof(I));
    }
    // a value table, converted to the program's dtype
    int upload(std::vector<double> v, int dtype) {
        if (dtype != GAAST_F32) return upload_bytes(v.data(), v.size(), sizeof(double));
        const std::vector<float> f(v.begin(), v.end());
        return upload_bytes(f.data(), f.size(), sizeof(float));
    }

private:
    int upload_bytes(const void* src, size_t n, size_t elem) {
        *this = DevTable();
        if (!n) return GAAST_OK;
        HIP_TRY(hipMalloc(&ptr, n * elem));
        count = n;
        HIP_TRY(hipMemcpy(ptr, src, n * elem, hipMemcpyHostToDevice));
        return GAAST_OK;
    }
};

// ---- run-time compiled kernels and their cache (include/gaast_hip.h: gaast_hip_jit_cache_*) ------------------------------
// One compiled kernel of the process: the code image, the module loaded from it and its entry point.  Every program whose
// generated source, entry point and compile options hash to the same key holds the same entry; the module is unloaded when
// the last of them is destroyed (gaast_hip_program_destroy has synchronised the stream by then).
struct JitEntry {
    jitcache::Digest key{};
    // HIP's header does not say that hipModuleLoadData copies the image: it stays alive for as long as the module does.
    // (Members are destroyed after the destructor's body: the module is unloaded before the image is freed.)
    std::vector<char> code;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    JitEntry() = default;
    JitEntry(const JitEntry&) = delete;
    JitEntry& operator=(const JitEntry&) = delete;
    ~JitEntry();
};

enum { JIT_COMPILED, JIT_MEMORY_HITS, JIT_DISK_HITS, JIT_DISK_STORES, JIT_DISK_REJECTED, JIT_LIVE_MODULES, JIT_N_COUNTERS };
static_assert(JIT_N_COUNTERS == GAAST_JIT_CACHE_N_COUNTERS && JIT_LIVE_MODULES == GAAST_JIT_CACHE_LIVE_MODULES, "counter order of gaast_hip.h");

// Never destroyed: a program may be destroyed (and its entries with it) while the process is on its way out
struct JitCache {
    std::mutex mutex;                                               // guards live and dir
    std::map<jitcache::Digest, std::weak_ptr<JitEntry>> live;       // the in-process level: always on
    std::string dir;                                                // the directory level: off while empty
    std::string compiler;                                           // hiprtcVersion, asked once
    std::atomic<int64_t> counters[JIT_N_COUNTERS] = {};
};
JitCache& jit_cache() {
    static JitCache* c = new JitCache;
    return *c;
}

JitEntry::~JitEntry() {
    if (module) {
        (void)hipModuleUnload(module);
        jit_cache().counters[JIT_LIVE_MODULES]--;
    }
    JitCache& c = jit_cache();
    std::lock_guard<std::mutex> lock(c.mutex);
    auto it = c.live.find(key);
    if (it != c.live.end() && it->second.expired()) c.live.erase(it);   // (not a newer entry under the same key)
}

// A program's handle on a compiled kernel
struct JitKernel {
    std::shared_ptr<JitEntry> entry;
    hipFunction_t fn = nullptr;   // entry->fn
    JitKernel() = default;
    explicit JitKernel(std::shared_ptr<JitEntry> e) : entry(std::move(e)), fn(entry ? entry->fn : nullptr) {}
    explicit operator bool() const { return fn != nullptr; }
};

}  // namespace

struct gaast_hip_mv_s {
    Layout layout;
    int64_t batch = 0;
    int dtype = GAAST_F64;
    int64_t row_stride = 0;  // elements
    void* ptr = nullptr;
    bool owns = false;
};

namespace {
// The compounds C_0(M) ... C_n(M) of a linear map on the device, in the dtype they are applied in (kernels_linmap.hip.hpp)
struct LinmapDev {
    int n = 0;
    int dtype = GAAST_F64;
    DevTable mats;
    std::vector<int> moff;            // grade k's matrix at element moff[k]
    int mat_total = 0;
    int small_blocks_per_cu = 1;      // k_linmap_small: resident workgroups per CU (persistent grid)
};

// One launch of a program: the plan's step it runs and what gaast_hip_program_create made of it on the device.  One group per
// launcher (its prepare_* / run_* pair): the step's tables on the device, under the names of their host images in Step (those
// are dropped after the upload), and the launch configuration, fixed once by prepare_*.  The groups of the other launchers
// stay empty.
struct Launch {
    Step s;
    int n = 0;                 // dimension of the algebra the kernel runs in (parity-pure dense products: n - 1)
    struct { DevTable axpy_map, flip_offsets; } trivial;   // AXPY, FLIP (SUNARY has no table)
    struct {   // DUAL
        DevTable segs, neg;
        int col_shift = 8;              // log2 of the components a workgroup of k_dual covers
    } dual;
    struct {   // INVERSE
        DevTable a_off, res_off, neg, weight;
        const void* kernel = nullptr;   // k_mv_inverse<T, N>
    } inv;
    struct {   // GEXP, GEXP_ADJ, GEXP_JVP, GEXP_ADJ2
        DevTable a_off, res_off, g_off, h_off, neg, neg_l, neg_r, weight;
        const void* kernel = nullptr;   // k_mv_gexp<T, N> / k_mv_gexp_adj<T, N> / k_mv_gexp_jvp<T, N> / k_mv_gexp_adj2<T, N>
    } gexp;
    struct {   // GSQRT, GSQRT_ADJ, GSQRT_JVP (g_off: the tangent's offsets, neg_r: the sign words of the right-multiplication matrix)
        DevTable a_off, res_off, g_off, neg, neg_l, neg_r, weight;
        const void* kernel = nullptr;   // k_mv_gsqrt<T, N> / k_mv_gsqrt_adj<T, N> / k_mv_gsqrt_jvp<T, N>
    } gsqrt;
    struct {   // GLOG, GLOG_ADJ, GLOG_JVP (as GSQRT_JVP)
        DevTable a_off, res_off, g_off, neg, neg_l, neg_r, weight;
        const void* kernel = nullptr;   // k_mv_glog<T, N> / k_mv_glog_adj<T, N> / k_mv_jvp_glog<T, N>
    } glog;
    struct {   // GLOG_ADJ2 (neg_m: the sign words of the right-multiplication matrix)
        DevTable a_off, res_off, g_off, h_off, neg, neg_l, neg_r, neg_m, weight;
        const void* kernel = nullptr;   // k_mv_adj2_glog<T, N>
    } glog2;
    struct {   // PRODUCT_CSR: k_product_csr, k_product_ell, k_product_ell_chain or the specialised gaast_chain
        DevTable row_start, row_out, entries, coeff;
        struct { DevTable entries, row_map; } pre;        // k_product_ell_chain: the first list
        struct { DevTable ent1, pos1, ent2, out2; } cj;   // gaast_chain: tables of its own
        size_t bytes_per_item = 0;      // k_product_csr / k_product_ell: LDS of one staged item
        int csr_items = 0;              // k_product_csr: items per workgroup when the batch allows
        const void* ell[4] = {nullptr, nullptr, nullptr, nullptr};   // k_product_ell<T, 1 << i, ...> by i = log2(items per pass)
        int ell_max_log2 = 0;           // ... the largest i built: picked by batch
        int chain_threads = 0;          // k_product_ell_chain / gaast_chain: workgroup size
        size_t chain_bytes = 0;         // k_product_ell_chain: dynamic LDS of a launch
        int chain_blocks_per_cu = 0;    // k_product_ell_chain / gaast_chain: resident workgroups per CU
    } list;
    struct {   // PRODUCT_DENSE
        DevTable left_map, right_map, out_map, spinor_out_map, left_scale, right_scale, out_scale;
        struct { DevTable row_start, entries, coeff, row_map, row_scale; } pre;   // chained: the list ahead of the product
        const void* general = nullptr;       // any rows
        const void* prefetch = nullptr;      // register-prefetch staging (k_gp_mfma6: its straight-line item loop): by the rows bound
        const void* whole_rows = nullptr;    // ... with straight-line result stores
        const void* spinor_fast = nullptr;   // k_gp_spinor12s: full, aligned rows on both sides and in the result
        int threads = 0;
        int items_per_block = 0;
        size_t bytes = 0;                // dynamic LDS of a launch
        size_t pre_scratch_bytes = 0;    // chained: where the list's operand rows sit in that LDS (after the kernel's images)
        int blocks_per_cu = 0;           // > 0: persistent workgroups, this many resident per CU
    } dense;
    struct {   // REDUCE_SCALE
        DevTable ent1, coeff1, ent2, coeff2, sign_words;
        const void* wave = nullptr;      // k_reduce_scale_wave<T, s.reduce.wave>, if built
        int blocks_per_cu = 0;           // k_reduce_scale: resident workgroups per CU
    } reduce;
    struct { DevTable sq, row_start, pairs, pair_coeff; } explog;
    struct {   // EXPLOG_ADJ
        DevTable sq;
        const void* kernel = nullptr;
        int lds_items = 0;               // items of a workgroup whose rows go through LDS; 0: the direct form
        size_t bytes_per_item = 0;       // LDS of one such item
    } adj;
    struct { DevTable ops, comp_off, out_off, coeff; } ew;
    struct { DevTable prog, phase_tab; std::vector<double> general; } fused;   // the interpreter's (general: passed by value)
    void* domain = nullptr;            // the program's domain-error counter (borrowed)
    const LinmapDev* linmap = nullptr; // LINMAP: the program's map (borrowed)
    // FUSED: the plan specialised through hiprtc, or a list chain (Step::cj); a FUSED step also gets the same source
    // compiled with floating-point contraction (l * r + acc as ONE fused multiply-add: fewer roundings than the reference, so
    // within the tolerance contract but not its bits): built only without GAAST_FLAG_EXACT_ORDER, launched only when an item's
    // arithmetic outweighs its bytes (run_fused -- in practice: operands shared by all items)
    JitKernel jit, jit_fma;
    std::string label;   // what the step is, then WHICH HIP kernel runs it (the name rocprofv3 reports)
    // which of a launch's kernels the most recent evaluation took (what its run_* returned): ELL: log2 of the items per pass;
    // dense: 0 general, 1 prefetch, 2 whole rows; spinor: 1 = the fast form; REDUCE_SCALE: 1 = the wave kernel; FUSED: 1 =
    // jit_fma; 0 where there is one kernel.  Host-side record for gaast_hip_program_launch_variant, -1 before any evaluation
    mutable int variant = -1;
};

struct MvFree {
    void operator()(gaast_hip_mv_t m) const;
};
using MvPtr = std::unique_ptr<gaast_hip_mv_s, MvFree>;
}  // namespace

struct gaast_hip_linmap_s {
    LinmapDev dev;
    std::vector<double> matrix;              // M as it was given: the compounds of M^T are built from it on first use
    std::unique_ptr<LinmapDev> transposed;   // C_k(M^T) = C_k(M)^T (gaast_hip_linmap_apply_transposed)
    // gaast_hip_linmap_matrix_vjp: the contraction's term table per grade mask of the rows, built when the mask is first seen
    struct VjpTable {
        DevTable terms, row_start;           // term words sorted by target (kernels_linmap.hip.hpp); n * n + 1 offsets
    };
    std::map<uint64_t, VjpTable> vjp_tables;
};

// Everything a program owns is freed through its members: gaast_hip_program_destroy synchronises the stream first
struct gaast_hip_program_s {
    Plan plan;                              // the shared data (layouts, inputs, buffers); its steps live on in `launches`
    std::vector<Launch> launches;
    std::vector<DevTable> const_rows;       // per input slot (empty for bound slots)
    std::vector<MvPtr> scratch;             // per node buffer, sized for scratch_batch
    int64_t scratch_batch = 0;
    DevTable domain;                        // exp / log extension: items refused by the domain check (unsigned long long)
    std::unique_ptr<LinmapDev> basis_in, basis_out;   // program in a non-orthonormal basis: C_k(Q^T) and C_k(Q) (LINMAP steps)
};

namespace {

int mv_alloc_impl(int dim, uint64_t mask, int64_t batch, int dtype, gaast_hip_mv_t* out) {
    auto* m = new gaast_hip_mv_s;
    m->layout = make_layout(dim, mask);
    m->batch = batch;
    m->dtype = dtype;
    m->row_stride = m->layout.row_len;
    m->owns = true;
    const size_t bytes = size_t(batch) * size_t(m->layout.row_len) * dtype_size(dtype);
    if (bytes) {
        hipError_t e = hipMalloc(&m->ptr, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(m->ptr, 0, bytes, g_stream);
        if (e != hipSuccess) {
            if (m->ptr) (void)hipFree(m->ptr);
            delete m;
            return set_err(GAAST_ERR_HIP, std::string("mv_alloc: ") + hipGetErrorString(e));
        }
    }
    *out = m;
    return GAAST_OK;
}

void mv_free_impl(gaast_hip_mv_t m) {
    if (!m) return;
    if (m->owns && m->ptr) (void)hipFree(m->ptr);
    delete m;
}
void MvFree::operator()(gaast_hip_mv_t m) const { mv_free_impl(m); }

struct Bound {  // a buffer resolved for one eval call
    void* ptr;
    int64_t stride;
};

// kernels whose dynamic LDS exceeds the 64 KiB default need the attribute raised, once
int allow_lds(const void* kern, size_t lds) {
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    return GAAST_OK;
}

int resident_blocks(const void* kern, int threads, size_t lds, int* per_cu) {
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, threads, lds));
    if (*per_cu < 1) *per_cu = 1;
    return GAAST_OK;
}

// after a kernel launch
int launch_status() {
    HIP_TRY(hipGetLastError());
    return GAAST_OK;
}

// grid of a persistent kernel: a workgroup per group of items, at most the `per_cu` workgroups per CU that are resident at once
// (per_cu <= 0: not persistent, every group gets its workgroup)
int64_t persistent_grid(int64_t groups, int per_cu) {
    return per_cu > 0 ? std::min<int64_t>(groups, int64_t(g_num_cu) * per_cu) : groups;
}

int grid_for(int64_t total, int block) {   // grid-stride beyond 8 blocks per CU
    return int(std::max<int64_t>(1, persistent_grid((total + block - 1) / block, 8)));
}

// 16-byte vector loads and stores of rows: base pointer and row pitch are multiples of 16 bytes
template <typename T>
bool rows_aligned16(const Bound& rows) {
    return reinterpret_cast<uintptr_t>(rows.ptr) % 16 == 0 && (size_t(rows.stride) * sizeof(T)) % 16 == 0;
}

// A kernel chosen at gaast_hip_program_create is kept as its address; launch_kernel gives it its type back, from the arguments
template <typename K>
const void* kernel_address(K kern) { return reinterpret_cast<const void*>(kern); }
template <typename... P>
void launch_kernel(const void* kern, int64_t blocks, int threads, size_t lds, const P&... params) {
    hipLaunchKernelGGL(reinterpret_cast<void (*)(P...)>(const_cast<void*>(kern)), dim3(unsigned(blocks)), dim3(unsigned(threads)), lds, g_stream, params...);
}

// Run-time values as template arguments, the one way a kernel family's instantiation is picked:
// static_bools(f, b0, b1, ...) = f(std::bool_constant<b0>, std::bool_constant<b1>, ...)
template <typename F>
auto static_bools(F&& f) { return f(); }
template <typename F, typename... Bs>
auto static_bools(F&& f, bool b, Bs... rest) {
    return b ? static_bools([&](auto... t) { return f(std::true_type{}, t...); }, rest...)
             : static_bools([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}
// static_int<V0, V1, ...>(v, f) = f(std::integral_constant<int, v>) if v is one of the Vs, else null: only the Vs are instantiated
template <int... Vs, typename F>
auto static_int(int v, F&& f) {
    std::common_type_t<decltype(f(std::integral_constant<int, Vs>{}))...> r = nullptr;
    (void)((v == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return r;
}

// ------------------------------------------------------------------------------------------
// Outermorphisms (kernels_linmap.hip.hpp): rows of layout `l` (dimension m.n) -> the same layout, `batch` items
// ------------------------------------------------------------------------------------------
constexpr int kLinmapSmallMaxDim = 6;
constexpr int kLinmapMaxDim = 14;   // the compounds at n = 14: C(28,14) ~ 40 M entries

size_t linmap_small_lds(const LinmapDev& m, int64_t row_len, size_t elem) {
    return (size_t((m.mat_total + 3) & ~3) + size_t(2 * kLinmapItems) * size_t(row_len + 1)) * elem;
}

// k_linmap_small's vector row I/O asks more than rows_aligned16: the rows are packed as well (pitch = row length)
template <typename T>
bool rows_packed_aligned16(const Bound& rows, int64_t row_len) { return rows.stride == row_len && rows_aligned16<T>(rows); }

template <typename T>
int launch_linmap(const LinmapDev& m, const Layout& l, const Bound& in, const Bound& out, int64_t batch) {
    if (batch <= 0 || l.row_len == 0) return GAAST_OK;
    LinmapArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.in = static_cast<const T*>(in.ptr);
    p.out = static_cast<T*>(out.ptr);
    p.mats = m.mats.as<T>();
    p.in_stride = in.stride;
    p.out_stride = out.stride;
    p.batch = batch;
    p.row_len = int(l.row_len);
    p.mat_total = m.mat_total;
    for (int k = 0; k <= m.n; ++k) {
        if (!((l.mask >> k) & 1ULL)) continue;
        const int len = int(n_choose_k(uint64_t(m.n), uint64_t(k)));
        const int g = p.n_grades++;
        p.goff[g] = int(l.offset(k));
        p.glen[g] = len;
        p.moff[g] = m.moff[size_t(k)];
        p.job0[g + 1] = p.job0[g] + (len + kLinmapBN - 1) / kLinmapBN;
        if (m.n <= kLinmapSmallMaxDim)
            for (int r = 0; r < len; ++r)
                p.comp[p.goff[g] + r] = uint32_t(p.goff[g]) | uint32_t(r) << 7 | uint32_t(len) << 13 | uint32_t(p.moff[g]) << 19;
    }
    p.n_jobs = p.job0[p.n_grades];
    if (m.n <= kLinmapSmallMaxDim) {
        p.in_vec = rows_packed_aligned16<T>(in, l.row_len);
        p.out_vec = rows_packed_aligned16<T>(out, l.row_len);
        const int64_t blocks = persistent_grid((batch + kLinmapItems - 1) / kLinmapItems, m.small_blocks_per_cu);
        hipLaunchKernelGGL(k_linmap_small<T>, dim3(unsigned(blocks)), dim3(256), linmap_small_lds(m, l.row_len, sizeof(T)), g_stream, p);
    } else {
        const int64_t tiles = std::min<int64_t>((batch + kLinmapBM - 1) / kLinmapBM, 65535);
        hipLaunchKernelGGL(k_linmap_mfma<T>, dim3(unsigned(p.n_jobs), unsigned(tiles)), dim3(256), 0, g_stream, p);
    }
    return launch_status();
}

const char* linmap_kernel_name(int n, int dtype) {
    if (n <= kLinmapSmallMaxDim) return dtype == GAAST_F32 ? "k_linmap_small<float>" : "k_linmap_small<double>";
    return dtype == GAAST_F32 ? "k_linmap_mfma<float>" : "k_linmap_mfma<double>";
}

// the compounds of `mat` (n x n, row-major) rounded to dtype, on the device (and in double, grade k at dev.moff[k], in *host).
// n <= kLinmapMaxDim.
int linmap_build(int n, const double* mat, int dtype, LinmapDev& dev, std::vector<double>* host = nullptr) {
    std::vector<std::vector<double>> c;
    compound_matrices(n, mat, n, c);
    dev.n = n;
    dev.dtype = dtype;
    dev.moff.assign(size_t(n + 1), 0);
    std::vector<double> all;
    for (int k = 0; k <= n; ++k) {
        dev.moff[size_t(k)] = int(all.size());
        all.insert(all.end(), c[size_t(k)].begin(), c[size_t(k)].end());
        std::vector<double>().swap(c[size_t(k)]);
    }
    dev.mat_total = int(all.size());
    if (host) *host = all;
    if (int st = dev.mats.upload(std::move(all), dtype)) return st;
    const size_t esz = dtype_size(dtype);
    if (n <= kLinmapSmallMaxDim) {
        const void* kern = dtype == GAAST_F32 ? reinterpret_cast<const void*>(&k_linmap_small<float>) : reinterpret_cast<const void*>(&k_linmap_small<double>);
        const size_t lds = linmap_small_lds(dev, kLinmapSmallComps, esz);   // the longest row
        if (int st = allow_lds(kern, lds)) return st;
        if (int st = resident_blocks(kern, 256, lds, &dev.small_blocks_per_cu)) return st;
    }
    return GAAST_OK;
}

// ------------------------------------------------------------------------------------------
// The launchers, one per kind of step (dispatch: prepare_launch, run_launch).  prepare_*: at gaast_hip_program_create, ONCE --
// the step's tables go to the device, the launch configuration is fixed (which kernel instantiation, block size, dynamic LDS,
// persistent grid) and `kernel` says which HIP kernel it is.  A step no kernel of this back end can run (operands beyond the
// LDS budget) makes program_create fail with UNIMPLEMENTED: an eval then either runs every step or none.  run_*: per
// evaluation -- the argument struct, the row form the bound rows allow, the launch; where a launcher has several kernels,
// *variant says which it took.
// ------------------------------------------------------------------------------------------
// The rows of one evaluation: what every buffer reference of a step resolves to
struct EvalRows {
    const gaast_hip_program_s* prog;
    const Layout* out_layout;
    // per input slot and for the result: the rows as the caller bound them, and as the steps of a program in a non-orthonormal
    // basis see them (moved into the orthogonal basis; the same rows in any other program)
    std::vector<Bound> callers, moved;
    Bound out_callers, out_moved;
    Bound at(BufRef r, Layout* lay, bool callers_rows = false) const {
        switch (r.kind) {
        case BufKind::NODE: {
            gaast_hip_mv_t m = prog->scratch[size_t(r.idx)].get();
            *lay = m->layout;
            return Bound{m->ptr, m->row_stride};
        }
        case BufKind::INPUT: *lay = prog->plan.input_layouts[size_t(r.idx)]; return (callers_rows ? callers : moved)[size_t(r.idx)];
        default: *lay = *out_layout; return callers_rows ? out_callers : out_moved;
        }
    }
};

// ... and the operands of one launch among them (null where the step has none)
struct Operands {
    Bound res{nullptr, 0}, a{nullptr, 0}, b{nullptr, 0}, c{nullptr, 0};
    Layout lres, la, lb;
    Bound pre_a{nullptr, 0}, pre_b{nullptr, 0}, scaled_row{nullptr, 0}, init{nullptr, 0};   // Step: pre.a, pre.b, reduce.x, cj.init_src
    const EvalRows* rows = nullptr;   // FUSED, ELEMENTWISE: they read by slot and by source list
};

template <typename T>
const char* type_name() { return std::is_same<T, double>::value ? "double" : "float"; }

// L.X from s.X: an index table as it is, a value table in the program's dtype T.  The first failure sticks.
template <typename T>
struct Upload {
    int status = GAAST_OK;
    template <typename I>
    void idx(DevTable& dev, std::vector<I>& host) { if (!status) status = dev.upload(std::move(host)); }
    void val(DevTable& dev, std::vector<double>& host) { if (!status) status = dev.upload(std::move(host), std::is_same<T, double>::value ? GAAST_F64 : GAAST_F32); }
};

// ---- AXPY, FLIP, SUNARY --------------------------------------------------------------------------------------------------
template <typename T>
int prepare_trivial(Launch& L, std::string& kernel) {
    Step& s = L.s;
    Upload<T> up;
    up.idx(L.trivial.axpy_map, s.axpy_map);
    up.idx(L.trivial.flip_offsets, s.flip_offsets);
    kernel = std::string(s.kind == Step::AXPY ? "k_axpy_map<" : s.kind == Step::FLIP ? "k_flip<" : "k_scalar_unary<") + type_name<T>() + ">";
    return up.status;
}

template <typename T>
int run_trivial(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (s.kind == Step::AXPY) {
        const int nm = int(L.trivial.axpy_map.count);
        hipLaunchKernelGGL(k_axpy_map<T>, dim3(grid_for(batch * nm, 256)), dim3(256), 0, g_stream,
                           static_cast<T*>(o.res.ptr), o.res.stride, static_cast<const T*>(o.a.ptr), o.a.stride,
                           L.trivial.axpy_map.as<uint32_t>(), nm, batch, s.beta);
    } else if (s.kind == Step::FLIP) {
        const int nm = int(L.trivial.flip_offsets.count);
        hipLaunchKernelGGL(k_flip<T>, dim3(grid_for(batch * nm, 256)), dim3(256), 0, g_stream,
                           static_cast<T*>(o.res.ptr), o.res.stride, L.trivial.flip_offsets.as<uint32_t>(), nm, batch);
    } else {
        hipLaunchKernelGGL(k_scalar_unary<T>, dim3(grid_for(batch, 256)), dim3(256), 0, g_stream,
                           static_cast<T*>(o.res.ptr), o.res.stride, s.sunary_off, s.sunary_op, batch);
    }
    return launch_status();
}

// ---- DUAL ----------------------------------------------------------------------------------------------------------------
template <typename T>
int prepare_dual(Launch& L, std::string& kernel) {
    Step& s = L.s;
    std::vector<uint32_t> segs;
    uint32_t first = 0;
    for (const Step::Dual::Seg& g : s.dual.segs) {
        segs.insert(segs.end(), {first, g.a_off, g.res_last, 0u});
        first += g.len;
    }
    L.dual.col_shift = 0;
    while (L.dual.col_shift < 8 && (1 << L.dual.col_shift) < s.dual.total) ++L.dual.col_shift;
    Upload<T> up;
    up.idx(L.dual.segs, segs);
    up.idx(L.dual.neg, s.dual.neg);
    kernel = std::string("k_dual<") + type_name<T>() + ">";
    return up.status;
}

template <typename T>
int run_dual(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0 || s.dual.total <= 0) return GAAST_OK;
    DualArgs<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.batch = batch;
    p.segs = L.dual.segs.as<uint32_t>();
    p.neg = L.dual.neg.as<uint32_t>();
    p.n_segs = int(L.dual.segs.count / 4);
    p.total = s.dual.total;
    p.col_shift = L.dual.col_shift;
    p.beta = s.beta;
    p.canon = s.canon_a;
    const int64_t per_block = 256 >> p.col_shift;
    const unsigned gx = unsigned((s.dual.total + (1 << p.col_shift) - 1) >> p.col_shift);
    const unsigned gy = unsigned(std::min<int64_t>((batch + per_block - 1) / per_block, 65535));
    hipLaunchKernelGGL(k_dual<T>, dim3(gx, gy), dim3(256), 0, g_stream, p);
    return launch_status();
}

// ---- INVERSE -------------------------------------------------------------------------------------------------------------
// (one kernel per (T, N): nothing is chosen at launch, the variant is 0)
template <typename T>
int prepare_inverse(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.inv;
    using Kern = void (*)(InverseArgs<T>);
    c.kernel = kernel_address(static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_inverse<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no inverse kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.neg, s.inv.neg); up.val(c.weight, s.inv.weight);
    kernel = std::string("k_mv_inverse<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_inverse(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    InverseArgs<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.batch = batch;
    p.a_off = L.inv.a_off.as<int32_t>();
    p.res_off = L.inv.res_off.as<int32_t>();
    p.neg = L.inv.neg.as<uint64_t>();
    p.weight = L.inv.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    p.dom = static_cast<unsigned long long*>(L.domain);
    const int64_t per_block = 256 / s.inv.N;
    launch_kernel(L.inv.kernel, persistent_grid((batch + per_block - 1) / per_block, 8), 256, 0, p);
    return launch_status();
}

// ---- GEXP, GEXP_ADJ ------------------------------------------------------------------------------------------------------
// (one kernel per (T, N) each: nothing is chosen at launch, the variant is 0)
template <typename T>
int prepare_gexp(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.gexp;
    const bool adj = s.kind == Step::GEXP_ADJ;
    using Kern = void (*)(GexpArgs<T>);
    c.kernel = kernel_address(adj ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gexp_adj<T, decltype(n)::value>; })
                                  : static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gexp<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no general-exponential kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.neg, s.inv.neg); up.val(c.weight, s.inv.weight);
    if (adj) {
        up.idx(c.g_off, s.inv.g_off); up.idx(c.neg_l, s.inv.adj_neg_l); up.idx(c.neg_r, s.inv.adj_neg_r);
    }
    kernel = std::string(adj ? "k_mv_gexp_adj<" : "k_mv_gexp<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_gexp(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    const bool adj = s.kind == Step::GEXP_ADJ;
    GexpArgs<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.cot = adj ? static_cast<const T*>(o.b.ptr) : nullptr;
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.cot_stride = adj ? o.b.stride : 0;
    p.batch = batch;
    p.a_off = L.gexp.a_off.as<int32_t>();
    p.res_off = L.gexp.res_off.as<int32_t>();
    p.g_off = L.gexp.g_off.as<int32_t>();
    p.neg = L.gexp.neg.as<uint64_t>();
    p.neg_l = L.gexp.neg_l.as<uint64_t>();
    p.neg_r = L.gexp.neg_r.as<uint64_t>();
    p.weight = L.gexp.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.wmax = T(s.inv.wmax);
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    p.dom = static_cast<unsigned long long*>(L.domain);
    const int64_t per_block = 256 / s.inv.N;
    launch_kernel(L.gexp.kernel, persistent_grid((batch + per_block - 1) / per_block, 8), 256, 0, p);
    return launch_status();
}

// ---- GEXP_JVP, GEXP_ADJ2 -------------------------------------------------------------------------------------------------
// (the second-order steps of the general exponential: one kernel per (T, N) each, the tables of GEXP_ADJ plus the tangent's offsets)
template <typename T>
int prepare_gexp2(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.gexp;
    const bool adj2 = s.kind == Step::GEXP_ADJ2;
    using Kern = void (*)(Gexp2Args<T>);
    c.kernel = kernel_address(adj2 ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gexp_adj2<T, decltype(n)::value>; })
                                   : static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gexp_jvp<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no general-exponential kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.h_off, s.inv.h_off); up.idx(c.neg, s.inv.neg); up.val(c.weight, s.inv.weight);
    if (adj2) {
        up.idx(c.g_off, s.inv.g_off); up.idx(c.neg_l, s.inv.adj_neg_l); up.idx(c.neg_r, s.inv.adj_neg_r);
    }
    kernel = std::string(adj2 ? "k_mv_gexp_adj2<" : "k_mv_gexp_jvp<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_gexp2(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    const bool adj2 = s.kind == Step::GEXP_ADJ2;
    Gexp2Args<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.cot = adj2 ? static_cast<const T*>(o.b.ptr) : nullptr;
    p.tan = static_cast<const T*>(o.c.ptr);
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.cot_stride = adj2 ? o.b.stride : 0;
    p.tan_stride = o.c.stride;
    p.batch = batch;
    p.a_off = L.gexp.a_off.as<int32_t>();
    p.res_off = L.gexp.res_off.as<int32_t>();
    p.g_off = L.gexp.g_off.as<int32_t>();
    p.h_off = L.gexp.h_off.as<int32_t>();
    p.neg = L.gexp.neg.as<uint64_t>();
    p.neg_l = L.gexp.neg_l.as<uint64_t>();
    p.neg_r = L.gexp.neg_r.as<uint64_t>();
    p.weight = L.gexp.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.wmax = T(s.inv.wmax);
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    const int64_t per_block = 256 / s.inv.N;
    const int per_cu = !adj2 ? 8 : sizeof(T) == 8 ? 2 : 4;   // (what the static LDS of k_mv_gexp_adj2 leaves resident on a CU)
    launch_kernel(L.gexp.kernel, persistent_grid((batch + per_block - 1) / per_block, per_cu), 256, 0, p);
    return launch_status();
}

// ---- GSQRT, GSQRT_ADJ ----------------------------------------------------------------------------------------------------
// (one kernel per (T, N) each, chosen by step kind and N: nothing is chosen at launch, the variant is 0)
template <typename T>
int prepare_gsqrt(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.gsqrt;
    const bool adj = s.kind == Step::GSQRT_ADJ, jvp = s.kind == Step::GSQRT_JVP;
    using Kern = void (*)(GsqrtArgs<T>);
    c.kernel = kernel_address(jvp   ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gsqrt_jvp<T, decltype(n)::value>; })
                              : adj ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gsqrt_adj<T, decltype(n)::value>; })
                                    : static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_gsqrt<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no general-square-root kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.neg, s.inv.neg); up.val(c.weight, s.inv.weight);
    if (adj) {
        up.idx(c.g_off, s.inv.g_off); up.idx(c.neg_l, s.inv.adj_neg_l); up.idx(c.neg_r, s.inv.adj_neg_r);
    }
    if (jvp) {   // (the tangent's offsets and the right-multiplication words travel in the cotangent's and ADJR's places)
        up.idx(c.g_off, s.inv.h_off); up.idx(c.neg_r, s.inv.rmul_neg);
    }
    kernel = std::string(jvp ? "k_mv_gsqrt_jvp<" : adj ? "k_mv_gsqrt_adj<" : "k_mv_gsqrt<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_gsqrt(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    const bool adj = s.kind == Step::GSQRT_ADJ, jvp = s.kind == Step::GSQRT_JVP;
    GsqrtArgs<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.cot = adj ? static_cast<const T*>(o.b.ptr) : jvp ? static_cast<const T*>(o.c.ptr) : nullptr;
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.cot_stride = adj ? o.b.stride : jvp ? o.c.stride : 0;
    p.batch = batch;
    p.a_off = L.gsqrt.a_off.as<int32_t>();
    p.res_off = L.gsqrt.res_off.as<int32_t>();
    p.g_off = L.gsqrt.g_off.as<int32_t>();
    p.neg = L.gsqrt.neg.as<uint64_t>();
    p.neg_l = L.gsqrt.neg_l.as<uint64_t>();
    p.neg_r = L.gsqrt.neg_r.as<uint64_t>();
    p.weight = L.gsqrt.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    p.dom = static_cast<unsigned long long*>(L.domain);
    const int64_t per_block = 256 / s.inv.N;
    launch_kernel(L.gsqrt.kernel, persistent_grid((batch + per_block - 1) / per_block, 8), 256, 0, p);
    return launch_status();
}

// ---- GLOG, GLOG_ADJ ----------------------------------------------------------------------------------------------------
// (one kernel per (T, N) each, chosen by step kind and N: nothing is chosen at launch, the variant is 0)
template <typename T>
int prepare_glog(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.glog;
    const bool adj = s.kind == Step::GLOG_ADJ, jvp = s.kind == Step::GLOG_JVP;
    using Kern = void (*)(GlogArgs<T>);
    c.kernel = kernel_address(jvp   ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_jvp_glog<T, decltype(n)::value>; })
                              : adj ? static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_glog_adj<T, decltype(n)::value>; })
                                    : static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_glog<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no general-logarithm kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.neg, s.inv.neg); up.val(c.weight, s.inv.weight);
    if (adj) {
        up.idx(c.g_off, s.inv.g_off); up.idx(c.neg_l, s.inv.adj_neg_l); up.idx(c.neg_r, s.inv.adj_neg_r);
    }
    if (jvp) {   // (as prepare_gsqrt)
        up.idx(c.g_off, s.inv.h_off); up.idx(c.neg_r, s.inv.rmul_neg);
    }
    kernel = std::string(jvp ? "k_mv_jvp_glog<" : adj ? "k_mv_glog_adj<" : "k_mv_glog<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_glog(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    const bool adj = s.kind == Step::GLOG_ADJ, jvp = s.kind == Step::GLOG_JVP;
    GlogArgs<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.cot = adj ? static_cast<const T*>(o.b.ptr) : jvp ? static_cast<const T*>(o.c.ptr) : nullptr;
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.cot_stride = adj ? o.b.stride : jvp ? o.c.stride : 0;
    p.batch = batch;
    p.a_off = L.glog.a_off.as<int32_t>();
    p.res_off = L.glog.res_off.as<int32_t>();
    p.g_off = L.glog.g_off.as<int32_t>();
    p.neg = L.glog.neg.as<uint64_t>();
    p.neg_l = L.glog.neg_l.as<uint64_t>();
    p.neg_r = L.glog.neg_r.as<uint64_t>();
    p.weight = L.glog.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.wmax = T(s.inv.wmax);
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    p.dom = static_cast<unsigned long long*>(L.domain);
    const int64_t per_block = 256 / s.inv.N;
    launch_kernel(L.glog.kernel, persistent_grid((batch + per_block - 1) / per_block, 8), 256, 0, p);
    return launch_status();
}

// ---- GLOG_ADJ2 -----------------------------------------------------------------------------------------------------------
// (the second-order adjoint of the general logarithm: one kernel per (T, N), the tables of GLOG_ADJ and of GLOG_JVP together)
template <typename T>
int prepare_glog_adj2(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.glog2;
    using Kern = void (*)(GlogAdj2Args<T>);
    c.kernel = kernel_address(static_int<2, 4, 8, 16, 32, 64>(s.inv.N, [](auto n) -> Kern { return k_mv_adj2_glog<T, decltype(n)::value>; }));
    if (!c.kernel) return set_err(GAAST_ERR_UNIMPLEMENTED, "no general-logarithm kernel for " + std::to_string(s.inv.N) + " blades");
    Upload<T> up;
    up.idx(c.a_off, s.inv.a_off); up.idx(c.res_off, s.inv.res_off); up.idx(c.g_off, s.inv.g_off); up.idx(c.h_off, s.inv.h_off);
    up.idx(c.neg, s.inv.neg); up.idx(c.neg_l, s.inv.adj_neg_l); up.idx(c.neg_r, s.inv.adj_neg_r); up.idx(c.neg_m, s.inv.rmul_neg);
    up.val(c.weight, s.inv.weight);
    kernel = std::string("k_mv_adj2_glog<") + type_name<T>() + "," + std::to_string(s.inv.N) + ">";
    return up.status;
}

template <typename T>
int run_glog_adj2(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    if (batch <= 0) return GAAST_OK;
    GlogAdj2Args<T> p;
    p.res = static_cast<T*>(o.res.ptr);
    p.in = static_cast<const T*>(o.a.ptr);
    p.cot = static_cast<const T*>(o.b.ptr);
    p.tan = static_cast<const T*>(o.c.ptr);
    p.res_stride = o.res.stride;
    p.in_stride = o.a.stride;
    p.cot_stride = o.b.stride;
    p.tan_stride = o.c.stride;
    p.batch = batch;
    p.a_off = L.glog2.a_off.as<int32_t>();
    p.res_off = L.glog2.res_off.as<int32_t>();
    p.g_off = L.glog2.g_off.as<int32_t>();
    p.h_off = L.glog2.h_off.as<int32_t>();
    p.neg = L.glog2.neg.as<uint64_t>();
    p.neg_l = L.glog2.neg_l.as<uint64_t>();
    p.neg_r = L.glog2.neg_r.as<uint64_t>();
    p.neg_m = L.glog2.neg_m.as<uint64_t>();
    p.weight = L.glog2.weight.as<T>();
    p.a_neg = s.inv.a_neg;
    p.wmax = T(s.inv.wmax);
    p.n = L.n;
    p.even = s.inv.even;
    p.beta = s.beta;
    const int64_t per_block = 256 / s.inv.N;
    const int per_cu = sizeof(T) == 8 ? 2 : 4;   // (what the static LDS of k_mv_adj2_glog leaves resident on a CU)
    launch_kernel(L.glog2.kernel, persistent_grid((batch + per_block - 1) / per_block, per_cu), 256, 0, p);
    return launch_status();
}

// ---- LINMAP --------------------------------------------------------------------------------------------------------------
// (nothing to prepare but the kernel's name; its operands are the caller's rows: run_launches)
template <typename T>
int run_linmap(const Launch& L, const Operands& o, int64_t batch) {
    const bool shared = L.s.a.kind == BufKind::INPUT && o.a.stride == 0;   // an input shared by every item: moved once
    return launch_linmap<T>(*L.linmap, o.la, o.a, o.res, shared ? 1 : batch);
}

// What the argument struct of every product kernel (CsrArgs, EllArgs, DenseArgs, SpinorArgs) holds under the same names
template <typename T, typename Args>
void product_operands(Args& q, const Step& s, const Operands& o, int64_t batch) {
    q.left = static_cast<const T*>(o.a.ptr);
    q.right = static_cast<const T*>(o.b.ptr);
    q.out = static_cast<T*>(o.res.ptr);
    q.left_stride = o.a.stride;
    q.right_stride = o.b.stride;
    q.out_stride = o.res.stride;
    q.canon_left = s.canon_a;
    q.canon_right = s.canon_b;
    q.beta = s.beta;
    q.batch = batch;
}

// ---- PRODUCT_CSR: a comp-mul list (CSR or ELL form), two chained lists, or the list chain specialised through hiprtc -------
template <typename T>
int prepare_list(Launch& L, const Layout& la, const Layout& lb, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.list;
    const std::string tn = type_name<T>();
    Upload<T> up;
    up.idx(c.row_start, s.list.row_start); up.idx(c.row_out, s.list.row_out); up.idx(c.entries, s.list.entries); up.val(c.coeff, s.list.coeff);
    if (L.jit) {   // the specialised kernel has tables of its own: cj, not pre
        up.idx(c.cj.ent1, s.cj.ent1); up.idx(c.cj.pos1, s.cj.pos1); up.idx(c.cj.ent2, s.cj.ent2); up.idx(c.cj.out2, s.cj.out2);
    } else {
        up.idx(c.pre.entries, s.pre.entries); up.idx(c.pre.row_map, s.pre.row_map);
    }
    if (up.status) return up.status;
    const size_t per_item = size_t(la.row_len + lb.row_len) * sizeof(T);
    if (per_item > g_max_lds)
        return set_err(GAAST_ERR_UNIMPLEMENTED,
                       "product operands of " + std::to_string(per_item) + " bytes per item do not fit the " +
                           std::to_string(g_max_lds) + "-byte LDS of the list kernels (" + s.name + ")");
    if (L.jit) {
        // the chain (or single long-row list) specialised through hiprtc (plan_chain_jit.cpp: make_chain_jit): static LDS, persistent workgroups
        c.chain_threads = s.cj.threads;
        kernel = "gaast_chain<" + tn + ">[" + (s.cj.single ? "one list, " : "") + std::to_string(s.cj.ipb) + " items, " + std::to_string(s.cj.threads) + " threads" +
                  (s.cj.split > 1 ? ", rows in " + std::to_string(s.cj.split) + " slices: re-ordered sums" : "") +
                  (s.cj.fmt[1] >= 3 ? ", sign-sorted terms" : "") + "]";
        int per_cu = 0;
        HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, L.jit.fn, c.chain_threads, 0));
        c.chain_blocks_per_cu = per_cu < 1 ? 1 : per_cu;
        return GAAST_OK;
    }
    if (s.chain.side) {
        // two lists in one launch, the mid row in LDS (plan_passes.cpp: chain_list_into_list): IPB items per workgroup
        c.chain_bytes = size_t(s.chain.ent2_lds) + size_t(s.chain.item_stride) * size_t(s.chain.ipb) * sizeof(T);
        if (c.chain_bytes > g_max_lds) return set_err(kChainTooBig, "list chain does not fit in LDS (" + s.name + ")");
        const int64_t pairs2 = int64_t(c.row_out.count) * s.chain.ipb;
        c.chain_threads = int(std::min<int64_t>(512, std::max<int64_t>(256, (pairs2 + 63) / 64 * 64)));
        const void* kern = kernel_address(&k_product_ell_chain<T>);
        kernel = "k_product_ell_chain<" + tn + ">";
        if (int st = allow_lds(kern, c.chain_bytes)) return st;
        return resident_blocks(kern, c.chain_threads, c.chain_bytes, &c.chain_blocks_per_cu);   // persistent workgroups
    }
    c.bytes_per_item = per_item;
    if (s.list.ell_width > 0) {
        // items per pass over the list: as many as a 64 KiB share of LDS holds (at least one), at most 8
        const int fit = int((64 * 1024) / per_item);
        c.ell_max_log2 = fit >= 8 ? 3 : fit >= 4 ? 2 : fit >= 2 ? 1 : 0;
        using KernE = void (*)(EllArgs<T>);
        const KernE tab[2][4] = {{&k_product_ell<T, 1, false>, &k_product_ell<T, 2, false>, &k_product_ell<T, 4, false>, &k_product_ell<T, 8, false>},
                                 {&k_product_ell<T, 1, true>, &k_product_ell<T, 2, true>, &k_product_ell<T, 4, true>, &k_product_ell<T, 8, true>}};
        kernel = "k_product_ell<" + tn + ",1.." + std::to_string(1 << c.ell_max_log2) + "," + (s.list.ell_bytes ? "true" : "false") + ">";
        for (int l2 = 0; l2 <= c.ell_max_log2; ++l2) {
            c.ell[l2] = kernel_address(tab[s.list.ell_bytes ? 1 : 0][l2]);
            if (int st = allow_lds(c.ell[l2], per_item << l2)) return st;
        }
        return GAAST_OK;
    }
    // enough items per block to give 256 threads work, within a 64 KiB LDS budget
    const int n_rows = int(c.row_out.count);
    int items = int((256 + n_rows - 1) / (n_rows > 0 ? n_rows : 1));
    const size_t budget = 64 * 1024;
    if (per_item * size_t(items) > budget) items = int(budget / per_item);
    if (items < 1) items = 1;
    c.csr_items = items;
    kernel = "k_product_csr<" + tn + ">";
    return allow_lds(kernel_address(&k_product_csr<T>), per_item * size_t(items));
}

template <typename T>
int run_list(const Launch& L, const Operands& o, int64_t batch, int* variant) {
    const Step& s = L.s;
    const auto& c = L.list;
    const Bound &res = o.res, &a = o.a, &b = o.b;
    if (L.jit) {
        const bool mid_left = s.chain.side == 1, single = s.cj.single != 0;
        const Bound& other = single ? b : s.chain.alias ? o.pre_a : (mid_left ? b : a);
        // a single list: its left operand is staged as the "mid" row (pointer l1), its right one is list 2's own operand (r2)
        const void *l1 = single ? a.ptr : o.pre_a.ptr, *r1 = single ? nullptr : o.pre_b.ptr, *r2 = other.ptr;
        long long s_l1 = single ? a.stride : o.pre_a.stride, s_r1 = single ? 0 : o.pre_b.stride, s_r2 = other.stride, s_out = res.stride, nb = batch;
        void* optr = res.ptr;
        const void *e1 = c.cj.ent1.ptr, *p1 = c.cj.pos1.ptr, *e2 = c.cj.ent2.ptr, *o2 = c.cj.out2.ptr;
        const void* init = o.init.ptr;   // the folded copy's source, if any
        long long s_init = o.init.stride;
        void* args[] = {&l1, &s_l1, &r1, &s_r1, &r2, &s_r2, &optr, &s_out, &e1, &p1, &e2, &o2, &nb, &init, &s_init};
        const int64_t blocks = persistent_grid((batch + s.cj.ipb - 1) / s.cj.ipb, c.chain_blocks_per_cu);
        // (the argument block is copied into the dispatch packet at call time, like run_fused's)
        HIP_TRY(hipModuleLaunchKernel(L.jit.fn, unsigned(blocks), 1, 1, unsigned(c.chain_threads), 1, 1, 0, g_stream,
                                      args, nullptr));
    } else if (s.chain.side) {
        EllChainArgs<T> q;
        const bool mid_left = s.chain.side == 1;
        const Bound& other = mid_left ? b : a;
        const Layout& lo = mid_left ? o.lb : o.la;
        q.l1 = static_cast<const T*>(o.pre_a.ptr);
        q.r1 = static_cast<const T*>(o.pre_b.ptr);
        q.r2 = static_cast<const T*>(other.ptr);
        q.out = static_cast<T*>(res.ptr);
        q.l1_stride = o.pre_a.stride;
        q.r1_stride = o.pre_b.stride;
        q.r2_stride = other.stride;
        q.out_stride = res.stride;
        q.l1_len = s.pre.left_len;
        q.r1_len = s.pre.right_len;
        q.r2_len = int(lo.row_len);
        q.mid_len = s.chain.mid_len;
        q.canon_l1 = s.pre.canon_a;
        q.canon_r1 = s.pre.canon_b;
        q.canon_r2 = mid_left ? s.canon_b : s.canon_a;
        q.canon_mid = s.chain.canon_mid;
        q.ent1 = c.pre.entries.as<uint32_t>();
        q.pos1 = c.pre.row_map.as<uint32_t>();
        q.rows1 = int(c.pre.row_map.count);
        q.width1 = s.pre.width;
        q.ent2 = c.entries.as<uint32_t>();
        q.out2 = c.row_out.as<uint32_t>();
        q.rows2 = int(c.row_out.count);
        q.width2 = s.list.ell_width;
        q.mid_is_left = mid_left ? 1 : 0;
        q.r2_alias = s.chain.alias;
        q.mid_covered = s.chain.covered;
        q.beta = s.beta;
        q.ipb = s.chain.ipb;
        q.item_stride = s.chain.item_stride;
        q.batch = batch;
        q.ent2_lds_bytes = s.chain.ent2_lds;
        const int64_t blocks = persistent_grid((batch + s.chain.ipb - 1) / s.chain.ipb, c.chain_blocks_per_cu);
        hipLaunchKernelGGL(k_product_ell_chain<T>, dim3(unsigned(blocks)), dim3(unsigned(c.chain_threads)), c.chain_bytes, g_stream, q);
    } else if (s.list.ell_width > 0) {
        EllArgs<T> q;
        product_operands<T>(q, s, o, batch);
        q.left_len = int(o.la.row_len);
        q.right_len = int(o.lb.row_len);
        q.row_out = c.row_out.as<uint32_t>();
        q.entries = c.entries.as<uint32_t>();
        q.n_rows = int(c.row_out.count);
        q.width = s.list.ell_width;
        int l2 = c.ell_max_log2;
        while (l2 > 0 && (int64_t(1) << l2) > batch) --l2;
        *variant = l2;
        launch_kernel(c.ell[l2], (batch + (int64_t(1) << l2) - 1) >> l2, 256, c.bytes_per_item << l2, q);
    } else {
        CsrArgs<T> p;
        product_operands<T>(p, s, o, batch);
        p.left_len = int(o.la.row_len);
        p.right_len = int(o.lb.row_len);
        p.row_start = c.row_start.as<uint32_t>();
        p.row_out = c.row_out.as<uint32_t>();
        p.entries = c.entries.as<uint32_t>();
        p.coeff = c.coeff.as<T>();
        p.n_rows = int(c.row_out.count);
        p.items = int(std::min<int64_t>(c.csr_items, batch));
        const int64_t blocks = (batch + p.items - 1) / p.items;
        hipLaunchKernelGGL(k_product_csr<T>, dim3(unsigned(blocks)), dim3(256), c.bytes_per_item * size_t(p.items), g_stream, p);
    }
    return launch_status();
}

// ---- PRODUCT_DENSE: the matrix-core and vector-FMA families, the matrix-representation (spinor) kernels ---------------------
// staging / store mode of k_gp_mfma16x4 and k_gp_mfma7 as a template argument
template <int V>
using Mode = std::integral_constant<int, V>;

// the spinor kernels see a full row as a D x D matrix, D = 2^m, and stage two of them (rows one element apart)
int64_t spinor_matrix_len(int m) { return int64_t(1) << (2 * m); }
template <typename T>
size_t spinor_planes_bytes(int m) {
    const size_t D = size_t(1) << m, plane = (D * (D + 1) + 63) / 64 * 64;
    return (m == 6 ? 2 * plane + (sizeof(T) == 8 ? 0 : 16) : 2 * D * (D + 1)) * sizeof(T);   // k_gp_spinor12s: second plane 16 words further
}

template <typename T>
int prepare_dense(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.dense;
    const int n = L.n;
    Upload<T> up;
    up.idx(c.left_map, s.dense.left_map); up.idx(c.right_map, s.dense.right_map); up.idx(c.out_map, s.dense.out_map);
    up.idx(c.spinor_out_map, s.dense.spinor_out_map);
    up.val(c.left_scale, s.dense.left_scale); up.val(c.right_scale, s.dense.right_scale); up.val(c.out_scale, s.dense.out_scale);
    up.idx(c.pre.row_start, s.pre.row_start); up.idx(c.pre.entries, s.pre.entries); up.idx(c.pre.row_map, s.pre.row_map);
    up.val(c.pre.coeff, s.pre.coeff); up.val(c.pre.row_scale, s.pre.row_scale);
    if (up.status) return up.status;
    constexpr bool is_f64 = std::is_same<T, double>::value;
    const bool degenerate = s.dense.degenerate != 0, scaled = s.dense.scaled != 0, chained = s.dense.chained != 0;
    const std::string tn = type_name<T>();
    const std::string dg = degenerate ? "true" : "false";
    // (SCALED, CHAINED) template arguments as they appear in the kernel's name: ",true" = rescaled basis, ",false,true" = chained
    const std::string vs = chained ? (scaled ? ",true,true" : ",false,true") : (scaled ? ",true" : "");
    using KernD = void (*)(DenseArgs<T>);
    // k_gp_mfma16x4 / k_gp_mfma7, k(MODE, SCALED, CHAINED): general staging for any basis; register prefetch (full, contiguous,
    // 16-byte aligned rows at launch) and, on top, straight-line result stores (every blade produced, nothing accumulated) --
    // never for a rescaled basis (general diagonal metric), for a chained product in every mode
    auto staging_modes = [&](auto&& k) {
        c.general = kernel_address(static_bools([&](auto sc, auto ch) -> KernD { return k(Mode<0>{}, sc, ch); }, scaled, chained));
        c.prefetch = kernel_address(static_bools([&](auto ch) -> KernD { return k(Mode<1>{}, std::false_type{}, ch); }, chained && !scaled));
        c.whole_rows = kernel_address(static_bools([&](auto ch) -> KernD { return k(Mode<2>{}, std::false_type{}, ch); }, chained && !scaled));
    };
    bool persistent = true;   // as many workgroups as are resident at once (register- and LDS-limited) loop over the items
    if (s.dense.family != DenseFamily::SPINOR) {   // the workgroup of the family: dense_images.hip.hpp, where the plan builder sizes its chains from too
        const dense_images::Geometry g = dense_images::geometry(s.dense.family, n, int(sizeof(T)));
        c.threads = g.threads;
        c.items_per_block = g.items;
        c.bytes = g.bytes;
    }
    switch (s.dense.family) {
    case DenseFamily::SPINOR: {
        using KernS = void (*)(SpinorArgs);
        const int m = s.dense.spinor_m;
        c.bytes = spinor_planes_bytes<T>(m);
        const int lb5 = s.dense.spinor_lam_bit;
        KernS kern = nullptr;
        if (is_f64 && m == 6) kern = lb5 == 5 ? &k_gp_spinor12d<5> : lb5 == 4 ? &k_gp_spinor12d<4> : &k_gp_spinor12d<-1>;
        else if (is_f64 && m == 5) kern = lb5 == 4 ? &k_gp_spinor_wave1d<5, 4> : lb5 == 3 ? &k_gp_spinor_wave1d<5, 3> : &k_gp_spinor_wave1d<5, -1>;
        else if (is_f64) kern = lb5 == 3 ? &k_gp_spinor_wave1d<4, 3> : lb5 == 2 ? &k_gp_spinor_wave1d<4, 2> : &k_gp_spinor_wave1d<4, -1>;
        else if (m == 6) {
            kern = lb5 == 5 ? &k_gp_spinor12s<5, false> : lb5 == 4 ? &k_gp_spinor12s<4, false> : &k_gp_spinor12s<-1, false>;
            const KernS fast = lb5 == 5 ? &k_gp_spinor12s<5, true> : lb5 == 4 ? &k_gp_spinor12s<4, true> : &k_gp_spinor12s<-1, true>;
            c.spinor_fast = kernel_address(fast);
        }
        else if (m == 5) kern = lb5 == 4 ? &k_gp_spinor_wave1<5, 4> : lb5 == 3 ? &k_gp_spinor_wave1<5, 3> : &k_gp_spinor_wave1<5, -1>;
        else kern = lb5 == 3 ? &k_gp_spinor_wave1<4, 3> : lb5 == 2 ? &k_gp_spinor_wave1<4, 2> : &k_gp_spinor_wave1<4, -1>;
        c.general = kernel_address(kern);
        kernel = (m == 6 ? (is_f64 ? "k_gp_spinor12d<" : "k_gp_spinor12s<") : (is_f64 ? "k_gp_spinor_wave1d<" : "k_gp_spinor_wave1<") + std::to_string(m) + ",") +
                  std::to_string(lb5) + ">";
        c.threads = m == 6 ? 256 : 64;
        break;
    }
    case DenseFamily::MFMA32:
    case DenseFamily::MFMA32P:
        if constexpr (!is_f64) {
            const bool image_pairs = s.dense.family == DenseFamily::MFMA32P;
            if (c.bytes > g_max_lds) return set_err(GAAST_ERR_UNIMPLEMENTED, "dense product does not fit in LDS");
            if (image_pairs) {
                c.general = kernel_address(static_bools([&](auto dgn, auto sc, auto ch) -> KernD {
                    return static_int<10, 11, 12, 13>(n, [](auto nn) -> KernD {
                        return &k_gp_mfma32p<decltype(dgn)::value, decltype(nn)::value, decltype(sc)::value, decltype(ch)::value>;
                    });
                }, degenerate, scaled, chained));
                kernel = "k_gp_mfma32p<" + dg + "," + std::to_string(n) + vs + ">";
                break;
            }
            // (k_gp_mfma32 serves n = 14 only -- 16 waves and 128 KiB of LDS per item; n = 10 ... 13 run on k_gp_mfma32p)
            if (c.threads != 1024) return set_err(GAAST_ERR_UNIMPLEMENTED, "k_gp_mfma32 is built for n = 14 only");
            c.general = kernel_address(static_bools([](auto dgn, auto sc, auto ch) -> KernD {
                return &k_gp_mfma32<decltype(dgn)::value, 1024, decltype(sc)::value, decltype(ch)::value>;
            }, degenerate, scaled, chained));
            kernel = "k_gp_mfma32<" + dg + "," + std::to_string(c.threads) + vs + ">";
            persistent = false;
            break;
        }
        [[fallthrough]];   // (f64 has no such kernel)
    case DenseFamily::VECTOR_FMA: {
        if (c.bytes > g_max_lds)
            return set_err(GAAST_ERR_UNIMPLEMENTED, "dense product of dimension " + std::to_string(n) + " does not fit in LDS");
        c.general = kernel_address(static_bools([](auto dgn, auto wide, auto neglo, auto sc, auto ch) -> KernD {
            return &k_gp_dense<T, decltype(dgn)::value, decltype(wide)::value ? 512 : 256, decltype(neglo)::value, decltype(sc)::value, decltype(ch)::value>;
        }, degenerate, c.threads != 256, s.dense.neg_lo_all != 0, scaled, chained));
        kernel = "k_gp_dense<" + tn + "," + dg + "," + std::to_string(c.threads) + "," + (s.dense.neg_lo_all ? "true" : "false") + vs + ">";
        break;
    }
    case DenseFamily::MFMA16X4: {
        // k_gp_mfma16x4<T, DEG, n, MODE, SC, CH>: one wave per 16 result columns, one item per workgroup.  f64 runs n = 8 ... 12 on
        // it, f32 only n = 8, 9 (f32 at n >= 10 is k_gp_mfma32p's): the f32 instantiations for n = 10 ... 12 would be unreachable,
        // so they are not built.
        if (c.bytes > g_max_lds) return set_err(GAAST_ERR_UNIMPLEMENTED, "dense product does not fit in LDS");
        staging_modes([&](auto mode, auto sc, auto ch) -> KernD {
            auto of_n = [&](auto nn) -> KernD {
                return static_bools([](auto dgn) -> KernD {
                    return &k_gp_mfma16x4<T, decltype(dgn)::value, decltype(nn)::value, decltype(mode)::value, decltype(sc)::value, decltype(ch)::value>;
                }, degenerate);
            };
            if constexpr (is_f64) return static_int<8, 9, 10, 11, 12>(n, of_n);
            else return static_int<8, 9>(n, of_n);
        });
        if (!c.general || !c.prefetch || !c.whole_rows) return set_err(GAAST_ERR_UNIMPLEMENTED, "no k_gp_mfma16x4 instantiation for this dimension and value type");
        kernel = "k_gp_mfma16x4<" + tn + "," + dg + "," + std::to_string(n) + (scaled ? ",0" + vs + ">" : ",0|1|2" + vs + ">");   // staging / store mode: by alignment at launch
        break;
    }
    case DenseFamily::MFMA6: {
        // k_gp_mfma6<T>: one wave per item, persistent single-wave workgroups, 2 KiB (f32) / 4 KiB (f64) of operand images
        // general: any operands (partial grade sets, projected or accumulated results); prefetch: full operands, every blade produced,
        // nothing accumulated -- straight-line item loop with counted waits
        auto k6 = [](auto sc, auto straight) -> KernD { return &k_gp_mfma6<T, decltype(sc)::value, decltype(straight)::value>; };
        c.general = kernel_address(static_bools(k6, scaled, false));
        c.prefetch = kernel_address(static_bools(k6, scaled, true));
        kernel = "k_gp_mfma6<" + tn + (scaled ? ",true,0|1>" : ",false,0|1>");
        break;
    }
    case DenseFamily::MFMA7: {
        // k_gp_mfma7<T>: one wave per item, persistent single-wave workgroups
        staging_modes([](auto mode, auto sc, auto ch) -> KernD { return &k_gp_mfma7<T, decltype(mode)::value, decltype(sc)::value, decltype(ch)::value>; });
        kernel = "k_gp_mfma7<" + tn + (scaled ? ",0" + vs + ">" : ",0|1|2" + vs + ">");   // (null vectors: run-time, no instantiation of their own)
        break;
    }
    }
    if (chained) {
        // the list's operand rows of every item a workgroup stages at once, after the kernel's own images
        c.pre_scratch_bytes = (c.bytes + 15) / 16 * 16;
        const size_t items = size_t(c.items_per_block > 0 ? c.items_per_block : 1);
        // + the zero pair; the one-item matrix kernels keep the list's right row twice (+x, -x: a term's sign is an address)
        c.bytes = c.pre_scratch_bytes + (items * size_t(s.pre.left_len + s.pre.right_len + 1) + (items == 1 ? size_t(s.pre.right_len) : 0)) * sizeof(T);
        // The plan builder sizes a chain from the same geometry, against the LDS this back end is built for; the device's own limit is
        // only known here.  Beyond it gaast_hip_program_create rebuilds the program without chains.
        if (c.bytes > g_max_lds) return set_err(kChainTooBig, "chained product does not fit in LDS (" + s.name + ")");
    }
    for (const void* kern : {c.general, c.prefetch, c.whole_rows, c.spinor_fast})
        if (kern)
            if (int st = allow_lds(kern, c.bytes)) return st;
    if (!persistent) return GAAST_OK;
    // (the residency of the prefetch form where there is one; of the general form under a chain, whose LDS is the greater part)
    return resident_blocks(c.prefetch && !chained ? c.prefetch : c.general, c.threads, c.bytes, &c.blocks_per_cu);
}

template <typename T>
int run_dense(const Launch& L, const Operands& o, int64_t batch, int* variant) {
    const Step& s = L.s;
    const auto& c = L.dense;
    const Bound &res = o.res, &a = o.a, &b = o.b;
    if (s.dense.family == DenseFamily::SPINOR) {
        SpinorArgs q;
        product_operands<T>(q, s, o, batch);
        q.left_map = c.left_map.as<uint16_t>();
        q.right_map = c.right_map.as<uint16_t>();
        q.left_full = s.dense.left_full;
        q.right_full = s.dense.right_full;
        q.out_map = c.spinor_out_map.as<uint16_t>();
        q.out_full = s.dense.out_full;
        q.left_len = int(o.la.row_len);
        q.right_len = int(o.lb.row_len);
        q.has_alpha = s.dense.spinor_has_alpha;
        const int64_t full = spinor_matrix_len(s.dense.spinor_m);
        const bool fast = c.spinor_fast && s.dense.left_full && s.dense.right_full && s.dense.out_full && !s.beta && o.la.row_len == full && o.lb.row_len == full &&
                          rows_aligned16<T>(a) && rows_aligned16<T>(b) && rows_aligned16<T>(res);
        *variant = fast ? 1 : 0;
        launch_kernel(fast ? c.spinor_fast : c.general, persistent_grid(batch, c.blocks_per_cu), c.threads, c.bytes, q);
        return launch_status();
    }
    DenseArgs<T> p;
    product_operands<T>(p, s, o, batch);
    p.left_map = c.left_map.as<uint32_t>();
    p.right_map = c.right_map.as<uint32_t>();
    p.left_count = int(c.left_map.count);
    p.right_count = int(c.right_map.count);
    p.left_full = s.dense.left_full;
    p.right_full = s.dense.right_full;
    p.left_contig = s.dense.left_contig && rows_aligned16<T>(a);
    p.right_contig = s.dense.right_contig && rows_aligned16<T>(b);
    p.out_map = c.out_map.as<int32_t>();
    p.n = L.n;
    p.neg_hi = s.dense.neg_hi;
    p.zero_hi = s.dense.zero_hi;
    p.neg_lo = s.dense.neg_lo;
    p.left_signs = s.dense.left_signs;
    p.out_signs = s.dense.out_signs;
    p.right_signs = s.dense.right_signs;
    p.out_whole = dense_whole_row_stores(s);
    p.pre_left = p.pre_right = nullptr;
    p.pre_entries = nullptr;
    if (s.dense.chained) {   // the left operand is a comp-mul list over two other rows, evaluated in LDS while staging
        p.pre_left = static_cast<const T*>(o.pre_a.ptr);
        p.pre_right = static_cast<const T*>(o.pre_b.ptr);
        p.pre_left_stride = o.pre_a.stride;
        p.pre_right_stride = o.pre_b.stride;
        p.pre_left_len = s.pre.left_len;
        p.pre_right_len = s.pre.right_len;
        p.pre_canon_left = s.pre.canon_a;
        p.pre_canon_right = s.pre.canon_b;
        p.pre_row_start = c.pre.row_start.as<uint32_t>();
        p.pre_entries = c.pre.entries.as<uint32_t>();
        p.pre_coeff = c.pre.coeff.as<T>();
        p.pre_row_map = c.pre.row_map.as<uint32_t>();
        p.pre_row_scale = c.pre.row_scale.as<T>();
        p.pre_rows = int(c.pre.row_map.count);
        p.pre_width = s.pre.width;
        p.pre_scratch = int(c.pre_scratch_bytes / sizeof(T));
        p.left_count = 0;
    }
    p.left_scale = s.dense.scaled ? c.left_scale.as<T>() : nullptr;
    p.right_scale = s.dense.scaled ? c.right_scale.as<T>() : nullptr;
    p.out_scale = s.dense.scaled ? c.out_scale.as<T>() : nullptr;
    // register-prefetch staging: full, contiguous, aligned operand rows; a chained step computes its left operand from a list
    // (then only the right row is prefetched)
    bool prefetch = false;
    switch (s.dense.family) {
    case DenseFamily::MFMA6: prefetch = p.left_full && p.right_full && s.dense.out_full && !s.beta; break;   // k_gp_mfma6's straight-line instantiation
    case DenseFamily::MFMA7: prefetch = p.right_full && !s.dense.scaled && (s.dense.chained || p.left_full); break;   // one component per lane and load: no alignment needed
    case DenseFamily::MFMA16X4: prefetch = p.right_contig && p.right_full && !s.dense.scaled && (s.dense.chained || (p.left_contig && p.left_full)); break;
    default: break;   // (one form)
    }
    const bool whole_rows = prefetch && c.whole_rows && s.dense.out_full && !s.beta;   // straight-line result stores
    *variant = whole_rows ? 2 : prefetch ? 1 : 0;
    launch_kernel(whole_rows ? c.whole_rows : prefetch ? c.prefetch : c.general, persistent_grid((batch + c.items_per_block - 1) / c.items_per_block, c.blocks_per_cu),
                  c.threads, c.bytes, p);
    return launch_status();
}

// ---- REDUCE_SCALE --------------------------------------------------------------------------------------------------------
template <typename T>
int prepare_reduce(Launch& L, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.reduce;
    const std::string tn = type_name<T>();
    Upload<T> up;
    up.idx(c.ent1, s.reduce.ent1); up.val(c.coeff1, s.reduce.coeff1); up.idx(c.ent2, s.reduce.ent2); up.val(c.coeff2, s.reduce.coeff2);
    up.idx(c.sign_words, s.reduce.sign_words);
    if (up.status) return up.status;
    kernel = "k_reduce_scale<" + tn + ">";
    if (s.reduce.wave) {   // tolerance mode: one wave per item, the row read once -- taken at launch when the three rows are one (run_reduce)
        using KernW = void (*)(ReduceScaleArgs<T>, const uint32_t*);
        KernW kw = nullptr;
        if constexpr (sizeof(T) == 8) kw = static_int<1, 2, 4, 8, 16>(s.reduce.wave, [](auto w) -> KernW { return &k_reduce_scale_wave<T, decltype(w)::value>; });
        else kw = static_int<1, 2, 4, 8>(s.reduce.wave, [](auto w) -> KernW { return &k_reduce_scale_wave<T, decltype(w)::value>; });
        c.wave = kernel_address(kw);
        if (kw) kernel += " | k_reduce_scale_wave<" + tn + "," + std::to_string(s.reduce.wave) + "> (lane-parallel sums) when the rows are one";
        else s.reduce.wave = 0;
    }
    return resident_blocks(kernel_address(&k_reduce_scale<T>), 256, 0, &c.blocks_per_cu);
}

template <typename T>
int run_reduce(const Launch& L, const Operands& o, int64_t batch, int* variant) {
    const Step& s = L.s;
    const auto& c = L.reduce;
    const Bound &res = o.res, &a = o.a, &b = o.b, &x = o.scaled_row;
    ReduceScaleArgs<T> q;
    q.l1 = static_cast<const T*>(a.ptr);
    q.r1 = static_cast<const T*>(b.ptr);
    q.x = static_cast<const T*>(x.ptr);
    q.out = static_cast<T*>(res.ptr);
    q.l1_stride = a.stride;
    q.r1_stride = b.stride;
    q.x_stride = x.stride;
    q.out_stride = res.stride;
    q.ent1 = c.ent1.as<uint32_t>();
    q.coeff1 = c.coeff1.as<T>();
    q.ent2 = c.ent2.as<uint32_t>();
    q.coeff2 = c.coeff2.as<T>();
    q.n1 = int(c.ent1.count);
    q.n2 = int(c.ent2.count);
    q.canon_l1 = s.canon_a;
    q.canon_r1 = s.canon_b;
    q.canon_x = s.reduce.canon_x;
    q.canon_s = s.reduce.canon_s;
    q.s_is_left = s.reduce.s_is_left;
    q.op = s.reduce.op;
    q.batch = batch;
    if (s.reduce.wave && c.wave && a.ptr == b.ptr && a.ptr == x.ptr && a.stride == b.stride && a.stride == x.stride &&
        rows_aligned16<T>(a) && rows_aligned16<T>(res) && res.ptr != a.ptr) {
        // one wave per item, four per workgroup, persistent
        *variant = 1;
        launch_kernel(c.wave, persistent_grid((batch + 3) / 4, 8), 256, 0, q, c.sign_words.as<uint32_t>());
    } else {
        // sixteen items per wave, four waves per workgroup, persistent: as many workgroups as are resident at once
        const int64_t blocks = persistent_grid((batch + 63) / 64, c.blocks_per_cu > 0 ? c.blocks_per_cu : 8);
        hipLaunchKernelGGL(k_reduce_scale<T>, dim3(unsigned(blocks)), dim3(256), 0, g_stream, q);
    }
    return launch_status();
}

// ---- EXPLOG --------------------------------------------------------------------------------------------------------------
template <typename T>
int prepare_explog(Launch& L) {
    Step& s = L.s;
    Upload<T> up;
    up.val(L.explog.sq, s.explog.sq); up.idx(L.explog.row_start, s.explog.row_start); up.idx(L.explog.pairs, s.explog.pairs);
    up.val(L.explog.pair_coeff, s.explog.pair_coeff);
    return up.status;   // (its label names no kernel)
}

template <typename T>
int run_explog(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    ExpLogArgs<T> q;
    q.res = static_cast<T*>(o.res.ptr);
    q.arg = static_cast<const T*>(o.a.ptr);
    q.res_stride = o.res.stride;
    q.arg_stride = o.a.stride;
    q.op = s.explog.op;
    q.m = s.explog.m;
    q.m_res = s.explog.mres;
    q.arg_k = s.explog.arg_k;
    q.arg_0 = s.explog.arg_0;
    q.res_k = s.explog.res_k;
    q.res_0 = s.explog.res_0;
    q.sq = L.explog.sq.as<T>();
    q.row_start = L.explog.row_start.as<uint32_t>();
    q.pairs = L.explog.pairs.as<uint32_t>();
    q.pair_coeff = L.explog.pair_coeff.as<T>();
    q.n_rows = int(L.explog.row_start.count) - 1;
    q.dom = static_cast<unsigned long long*>(L.domain);
    q.batch = batch;
    hipLaunchKernelGGL(k_exp_log<T>, dim3(grid_for(batch, 256)), dim3(256), 0, g_stream, q);
    return launch_status();
}

// ---- EXPLOG_ADJ ----------------------------------------------------------------------------------------------------------
template <typename T>
int prepare_explog_adj(Launch& L, const Layout& la, const Layout& lb, std::string& kernel) {
    Step& s = L.s;
    auto& c = L.adj;
    Upload<T> up;
    up.val(c.sq, s.adj.sq);
    // the rows of a workgroup's items through LDS whenever at least a wave's worth of items fits 64 KiB (no attribute to raise,
    // several workgroups per CU); an item's rows `stride` elements apart, odd.  Otherwise the direct form.
    const size_t stride = size_t(la.row_len + lb.row_len) | 1;
    const size_t fit = (64 * 1024) / (stride * sizeof(T));
    c.lds_items = fit >= 256 ? 256 : int(fit / 64 * 64);
    c.bytes_per_item = stride * sizeof(T);
    c.kernel = s.adj.op == 0 ? kernel_address(&k_exp_log_adj<T, 0>) : kernel_address(&k_exp_log_adj<T, 1>);
    kernel = std::string("k_exp_log_adj<") + type_name<T>() + "," + std::to_string(s.adj.op) + ">" +
             (c.lds_items ? "[" + std::to_string(c.lds_items) + " items through LDS]" : "[direct rows]");
    return up.status;
}

template <typename T>
int run_explog_adj(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    const auto& c = L.adj;
    ExpLogAdjArgs<T> q;
    q.res = static_cast<T*>(o.res.ptr);
    q.arg = static_cast<const T*>(o.a.ptr);
    q.cot = static_cast<const T*>(o.b.ptr);
    q.res_stride = o.res.stride;
    q.arg_stride = o.a.stride;
    q.cot_stride = o.b.stride;
    q.m = s.adj.m;
    q.m_g = s.adj.mg;
    q.m_res = s.adj.res_k >= 0 ? s.adj.mres : 0;
    q.arg_k = s.adj.arg_k;
    q.arg_0 = s.adj.arg_0;
    q.g_k = s.adj.g_k;
    q.g_0 = s.adj.g_0;
    q.res_k = s.adj.res_k;
    q.res_0 = s.adj.res_0;
    q.arg_len = int(o.la.row_len);
    q.cot_len = int(o.lb.row_len);
    q.items = c.lds_items;
    q.lds_stride = int(c.bytes_per_item / sizeof(T));
    q.sq = c.sq.as<T>();
    q.batch = batch;
    const int per_block = c.lds_items ? c.lds_items : 256;   // the direct form: an item per thread
    launch_kernel(c.kernel, persistent_grid((batch + per_block - 1) / per_block, 8), 256, c.bytes_per_item * size_t(c.lds_items), q);
    return launch_status();
}

// ---- ELEMENTWISE: a run of element-wise arms (and the scaling product after it) in one pass: plan_passes.cpp: fuse_elementwise_runs ---
template <typename T>
int prepare_elementwise(Launch& L, std::string& kernel) {
    Step& s = L.s;
    Upload<T> up;
    up.idx(L.ew.ops, s.ew.ops); up.idx(L.ew.comp_off, s.ew.comp_off); up.idx(L.ew.out_off, s.ew.out_off); up.val(L.ew.coeff, s.ew.coeff);
    kernel = std::string("k_elementwise<") + type_name<T>() + (s.ew.n_ops <= 4 ? ",4>" : ",8>");
    return up.status;
}

template <typename T>
int run_elementwise(const Launch& L, const Operands& o, int64_t batch) {
    const Step& s = L.s;
    ElementwiseArgs<T> q;
    std::memset(&q, 0, sizeof(q));
    Layout unused;
    for (size_t i = 0; i < s.ew.src.size() && i < size_t(ELEMENTWISE_MAX_SRC); ++i) {
        const Bound src = o.rows->at(s.ew.src[i], &unused);
        q.src[i] = static_cast<const T*>(src.ptr);
        q.src_stride[i] = src.stride;
    }
    q.ops = L.ew.ops.as<uint32_t>();
    q.comp_off = L.ew.comp_off.as<uint32_t>();
    q.n_ops = s.ew.n_ops;
    q.n_comp = int(L.ew.comp_off.count);
    q.load_first = s.ew.load_first;
    q.batch = batch;
    if (s.ew.scale) {
        q.out = static_cast<T*>(o.res.ptr);
        q.out_stride = o.res.stride;
        q.out_off = L.ew.out_off.as<uint32_t>();
        q.coeff = L.ew.coeff.as<T>();
        q.scalar = static_cast<const T*>(o.b.ptr);
        q.scalar_stride = o.b.stride;
        q.scalar_off = s.ew.scalar_off;
        q.canon_v = s.ew.canon_v;
        q.canon_s = s.ew.canon_s;
        q.s_is_left = s.ew.s_is_left;
    } else {
        q.res = static_cast<T*>(o.res.ptr);
        q.res_stride = o.res.stride;
    }
    // x: the components (a thread keeps one), y: strides over the items -- enough workgroups to fill the chip a few times over
    const unsigned gx = unsigned((q.n_comp + 255) / 256);
    const int64_t want_y = std::max<int64_t>(1, int64_t(g_num_cu) * 16 / gx);
    const unsigned gy = unsigned(std::min<int64_t>(std::min<int64_t>((batch + 3) / 4, want_y), 65535));   // (a thread takes four items per step)
    if (q.n_ops <= 4) hipLaunchKernelGGL((k_elementwise<T, 4>), dim3(gx, gy), dim3(256), 0, g_stream, q);
    else hipLaunchKernelGGL((k_elementwise<T, ELEMENTWISE_MAX_OPS>), dim3(gx, gy), dim3(256), 0, g_stream, q);
    return launch_status();
}

// Loads a code image as a module of its own; null when HIP refuses it
std::shared_ptr<JitEntry> jit_load(const jitcache::Digest& key, std::vector<char> code, const char* entry) {
    auto e = std::make_shared<JitEntry>();
    e->key = key;
    e->code = std::move(code);
    if (hipModuleLoadData(&e->module, e->code.data()) != hipSuccess) {
        e->module = nullptr;
        return nullptr;
    }
    jit_cache().counters[JIT_LIVE_MODULES]++;
    if (hipModuleGetFunction(&e->fn, e->module, entry) != hipSuccess) return nullptr;
    return e;
}

// hiprtc itself: the code object of `source`, empty on any failure (*log says why)
std::vector<char> hiprtc_compile(const std::string& source, const std::vector<std::string>& options, std::string* log) {
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, source.c_str(), "gaast_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return {};
    std::vector<const char*> opts;
    for (const std::string& o : options) opts.push_back(o.c_str());
    const hiprtcResult res = hiprtcCompileProgram(prog, int(opts.size()), opts.data());
    if (res != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        log->assign(n, 0);
        if (n) hiprtcGetProgramLog(prog, &(*log)[0]);
        hiprtcDestroyProgram(&prog);
        return {};
    }
    size_t cs = 0;
    std::vector<char> code;
    bool got = hiprtcGetCodeSize(prog, &cs) == HIPRTC_SUCCESS && cs > 0;
    if (got) {
        code.resize(cs);
        got = hiprtcGetCode(prog, code.data()) == HIPRTC_SUCCESS;
    }
    hiprtcDestroyProgram(&prog);
    if (!got) {
        *log = "hiprtcGetCodeSize / hiprtcGetCode failed";
        return {};
    }
    return code;
}

// hiprtc specialisation of a fused plan or a list chain: an empty kernel on any failure (then the generic kernel stays in charge)
// (contract: the variant with fused multiply-adds, kept beside the exact one -- Launch::jit_fma)
// The ONE lookup point of the kernel cache: the modules alive in this process, then the directory (if one is set), then the
// compiler; only what the compiler produced is stored.  GAAST_FLAG_DEBUG_JIT_FAILS fails before either level is asked.
JitKernel jit_compile(const std::string& source, const char* entry, std::string* log, uint32_t flags, bool contract = false) {
    if (flags & GAAST_FLAG_DEBUG_JIT_FAILS) return {};
    JitCache& c = jit_cache();
    jitcache::KeyFields kf;
    kf.revision = GAAST_KERNELS_REV;
    kf.target = "gfx950";
    kf.options = {"--offload-arch=gfx950", "-O3", contract ? "-ffp-contract=fast" : "-ffp-contract=off"};
    kf.entry = entry;
    kf.source = source;
    std::string dir;
    {
        std::lock_guard<std::mutex> lock(c.mutex);
        if (c.compiler.empty()) {
            int major = 0, minor = 0;
            if (hiprtcVersion(&major, &minor) != HIPRTC_SUCCESS) return {};
            c.compiler = std::to_string(major) + "." + std::to_string(minor);
        }
        kf.compiler = c.compiler;
        dir = c.dir;
    }
    const jitcache::Digest key = jitcache::make_key(kf);
    {
        std::lock_guard<std::mutex> lock(c.mutex);
        auto it = c.live.find(key);
        if (it != c.live.end())
            if (std::shared_ptr<JitEntry> e = it->second.lock()) {
                c.counters[JIT_MEMORY_HITS]++;
                return JitKernel(std::move(e));
            }
    }
    std::shared_ptr<JitEntry> e;
    if (!dir.empty()) {
        std::vector<char> code;
        const jitcache::Load got = jitcache::load(dir, kf.revision, key, &code);
        if (got == jitcache::Load::Ok && (e = jit_load(key, std::move(code), entry)))
            c.counters[JIT_DISK_HITS]++;
        else if (got != jitcache::Load::Missing)
            c.counters[JIT_DISK_REJECTED]++;   // (a checked file HIP still refuses: as good as a bad one; replaced below)
    }
    if (!e) {
        std::vector<char> code = hiprtc_compile(source, kf.options, log);
        if (code.empty()) return {};
        c.counters[JIT_COMPILED]++;
        // a store that fails (no such directory, read-only, full disk) costs the next process a compilation, nothing else
        if (!dir.empty() && jitcache::store(dir, kf.revision, key, code.data(), code.size())) c.counters[JIT_DISK_STORES]++;
        e = jit_load(key, std::move(code), entry);
        if (!e) return {};
    }
    std::lock_guard<std::mutex> lock(c.mutex);
    c.live[key] = e;
    return JitKernel(std::move(e));
}

// When does the contracted variant of a specialised kernel pay?  An item costs ~2 vector instructions per comp-mul (4 cycles per
// wave instruction and SIMD, 64 items per wave, 1,024 SIMDs at 2.4 GHz) and `bytes` of HBM traffic at 8 TB/s; below 0.6 of the
// traffic time the arithmetic hides behind the rows (cl41: 336 comp-muls, 296 B: 0.46 -- measured 0.78-0.84 of HBM with the
// exact code), above it the vector ALUs are the bound (cl41 with one shared rotor: 168 B: 0.81 -- 79 % busy, 0.66 of HBM).
bool arithmetic_bound(uint64_t comp_muls, double bytes) {
    const double valu_ps = double(comp_muls) * 2.0 * 4.0 / 64.0 / (1024.0 * 2.4e9) * 1e12, hbm_ps = bytes / 8e12 * 1e12;
    return valu_ps > 0.6 * hbm_ps;
}

// ---- FUSED: the interpreter k_ast_fused, or the plan specialised through hiprtc (gaast_jit) --------------------------------------
// the slabs of the FUSED_ITEMS items of a k_ast_fused workgroup
template <typename T>
size_t fused_slabs_bytes(int slab) { return (size_t(slab) * FUSED_ITEMS + 8) * sizeof(T); }

template <typename T>
int prepare_fused(Launch& L) {
    Step& s = L.s;
    Upload<T> up;
    up.idx(L.fused.prog, s.fused.prog); up.idx(L.fused.phase_tab, s.fused.phase_tab);
    L.fused.general = std::move(s.fused.general);
    if (up.status || L.jit) return up.status;   // (the step's name says which kernel it is: compile_fused)
    return allow_lds(kernel_address(&k_ast_fused<T>), fused_slabs_bytes<T>(s.fused.slab));
}

template <typename T>
int run_jit(const Launch& L, const Operands& o, int64_t batch, int* variant) {
    const Step& s = L.s;
    const Plan& plan = o.rows->prog->plan;
    const std::vector<Bound>& in_bound = o.rows->moved;
    // argument block: (ptr, stride) per staged input image, then out, out stride, batch
    std::vector<void*> args;
    std::vector<const void*> ptrs(s.fused.inputs.size());
    std::vector<long long> strides(s.fused.inputs.size());
    for (size_t i = 0; i < s.fused.inputs.size(); ++i) {
        ptrs[i] = in_bound[size_t(s.fused.inputs[i].slot)].ptr;
        strides[i] = in_bound[size_t(s.fused.inputs[i].slot)].stride;
        args.push_back(&ptrs[i]);
        args.push_back(&strides[i]);
    }
    void* optr = o.res.ptr;
    long long ostride = o.res.stride, b = batch;
    args.push_back(&optr);
    args.push_back(&ostride);
    args.push_back(&b);
    void* dom = L.domain;
    if (plan.has_explog) args.push_back(&dom);
    const unsigned threads = unsigned(s.fused.jit_threads);
    const unsigned per_block = unsigned(s.fused.jit_items > 0 ? s.fused.jit_items : s.fused.jit_threads);   // (the slab-in-LDS form: 64 items per 512 threads)
    const int64_t blocks = persistent_grid((batch + per_block - 1) / per_block, std::min(s.fused.jit_persistent, 4));   // (jit_persistent = 0: a workgroup per group)
    // (the argument block -- args, ptrs, strides and the locals they point at -- only has to live until this call returns:
    //  hipModuleLaunchKernel copies the kernel arguments into the dispatch packet's kernarg segment at call time)
    hipFunction_t fn = L.jit.fn;
    if (L.jit_fma) {
        // tolerance mode: the rows this launch really moves -- an operand shared by all items moves none, and only then does the
        // contracted variant run (a program over batched operands only keeps the reference's bits by default, as before)
        double bytes = double(plan.out_layout.row_len) * sizeof(T);
        bool shared = false;
        for (size_t i = 0; i < s.fused.inputs.size(); ++i) {
            if (strides[i] != 0) bytes += double(plan.input_layouts[size_t(s.fused.inputs[i].slot)].row_len) * sizeof(T);
            else shared = true;
        }
        if (shared && arithmetic_bound(s.n_entries, bytes)) fn = L.jit_fma.fn;
    }
    *variant = fn == L.jit.fn ? 0 : 1;
    HIP_TRY(hipModuleLaunchKernel(fn, unsigned(blocks), 1, 1, threads, 1, 1, 0, g_stream, args.data(), nullptr));
    return GAAST_OK;
}

template <typename T>
int run_fused(const Launch& L, const Operands& o, int64_t batch, int* variant) {
    if (L.jit) return run_jit<T>(L, o, batch, variant);
    const Step& s = L.s;
    const Plan& plan = o.rows->prog->plan;
    FusedArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.prog = L.fused.prog.as<uint32_t>();
    p.phase_tab = L.fused.phase_tab.as<uint32_t>();
    p.n_phases = int(L.fused.phase_tab.count / (2 * FUSED_GROUPS));
    for (size_t i = 0; i < L.fused.general.size() && i < 6; ++i) p.coeff[i] = T(L.fused.general[i]);
    p.slab = s.fused.slab;
    p.zero_slot = s.fused.zero_slot;
    p.n_in = int(s.fused.inputs.size());
    for (int i = 0; i < p.n_in; ++i) {
        const Step::FusedInput& fi = s.fused.inputs[size_t(i)];
        p.in_ptr[i] = static_cast<const T*>(o.rows->moved[size_t(fi.slot)].ptr);
        p.in_stride[i] = o.rows->moved[size_t(fi.slot)].stride;
        p.in_len[i] = int(plan.input_layouts[size_t(fi.slot)].row_len);
        p.in_base[i] = fi.base;
        p.in_canon[i] = fi.canon;
    }
    p.out_ptr = static_cast<T*>(o.res.ptr);
    p.out_stride = o.res.stride;
    p.out_len = int(plan.out_layout.row_len);
    p.out_base = s.fused.out_base;
    p.batch = batch;
    const int64_t blocks = (batch + FUSED_ITEMS - 1) / FUSED_ITEMS;
    hipLaunchKernelGGL(k_ast_fused<T>, dim3(unsigned(blocks)), dim3(FUSED_THREADS), fused_slabs_bytes<T>(s.fused.slab), g_stream, p);
    return launch_status();
}
// ------------------------------------------------------------------------------------------
// Program creation (program_create_impl), phase by phase
// ------------------------------------------------------------------------------------------
// the plan of `desc` and one launch per step (plan.steps is left empty); a rebuild discards the launches made so far
int make_launches(const gaast_program_desc& desc, bool small_reg_slab, bool mirrored, gaast_hip_program_s& prog) {
    prog.launches.clear();
    prog.plan = Plan();
    try {
        build_plan(desc, prog.plan, small_reg_slab, mirrored);
    } catch (const std::exception& ex) {
        return set_err(GAAST_ERR_INVALID_PROGRAM, ex.what());
    }
    // valid in the reference, beyond this back end: refused whole, here, never half-evaluated
    if (!prog.plan.unsupported.empty()) return set_err(GAAST_ERR_UNIMPLEMENTED, prog.plan.unsupported);
    prog.launches.resize(prog.plan.steps.size());
    for (size_t i = 0; i < prog.launches.size(); ++i) prog.launches[i].s = std::move(prog.plan.steps[i]);
    prog.plan.steps.clear();
    return GAAST_OK;
}

// hiprtc specialisation of fused plans, before anything is uploaded.  True: the plan has to be rebuilt with *rebuild_flags /
// *small_reg_slab -- it can only run as the specialised kernel and the compiler is not available, or a register trial failed.
bool compile_fused(gaast_hip_program_s& prog, uint32_t flags, uint32_t* rebuild_flags, bool* small_reg_slab) {
    bool rebuild = false;
    for (Launch& L : prog.launches) {
        Step& s = L.s;
        if (s.kind != Step::FUSED || s.fused.jit_source.empty()) continue;
        if (flags & GAAST_FLAG_DEBUG_KEEP_JIT_SOURCE) prog.plan.jit_source_kept += s.fused.jit_source;
        std::string log;
        L.jit = jit_compile(s.fused.jit_source, "gaast_jit", &log, flags);
        if (L.jit)
            s.name = "ast_jit" + s.name.substr(s.name.find('[')) + (s.fused.jit_items ? " slab in LDS" : "");
        else if (!log.empty())
            g_err = "hiprtc: " + log;  // informational: the interpreter kernel (or an unfused plan) runs instead
        bool trial_failed = false;
        if (L.jit && s.fused.jit_reg_trial) {
            // a slab beyond 160 / 200 elements in registers, on trial (plan_fused.cpp: SlabLayout): the compiled kernel has to leave two
            // waves per SIMD (eight single-wave workgroups per CU), else the plan is rebuilt with the slabs in LDS
            int per_cu = 0;
            trial_failed = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, L.jit.fn, s.fused.jit_threads, 0) != hipSuccess ||
                           per_cu * (s.fused.jit_threads / 64) < 8;
            if (trial_failed) rebuild = *small_reg_slab = true;
        }
        // tolerance mode, one item per thread, and arithmetic-bound at least when every operand is shared by all items: the
        // contracted variant too (run_jit picks per launch, by the operands bound)
        if (L.jit && !trial_failed && !(flags & GAAST_FLAG_EXACT_ORDER) && !s.fused.jit_items && !prog.plan.has_explog && !prog.plan.has_explog_adj &&
            arithmetic_bound(s.n_entries, double(prog.plan.out_layout.row_len) * dtype_size(prog.plan.dtype))) {
            std::string log2;
            L.jit_fma = jit_compile(s.fused.jit_source, "gaast_jit", &log2, flags, true);
            if (L.jit_fma) s.name += " | fused multiply-adds under shared operands";
        }
        std::string().swap(s.fused.jit_source);
        if (!L.jit && s.fused.jit_only) {
            rebuild = true;
            *rebuild_flags |= GAAST_FLAG_NO_JIT;
        }
    }
    return rebuild;
}

// list chains specialised per program; on any failure the generic k_product_ell_chain stays in charge
void compile_chains(gaast_hip_program_s& prog, uint32_t flags) {
    std::vector<Launch>& ls = prog.launches;
    std::vector<char> drop(ls.size(), 0);
    for (size_t i = 0; i < ls.size(); ++i) {
        Step& s = ls[i].s;
        if (!s.cj.on) continue;
        if (flags & GAAST_FLAG_DEBUG_KEEP_JIT_SOURCE) prog.plan.jit_source_kept += s.cj.source;
        std::string log;
        ls[i].jit = jit_compile(s.cj.source, "gaast_chain", &log, flags);
        if (!ls[i].jit && !log.empty()) g_err = "hiprtc: " + log;
        std::string().swap(s.cj.source);
        if (!ls[i].jit) {
            s.cj.single = s.cj.fold_prev = 0;
            s.cj.init_src = BufRef();
        } else if (s.cj.fold_prev && i > 0) {   // the copy_grades_from step before a single list is evaluated by the specialised kernel
            drop[i - 1] = 1;
            s.name += " <- " + ls[i - 1].s.name;
        }
    }
    std::vector<Launch> kept;
    for (size_t i = 0; i < ls.size(); ++i)
        if (!drop[i]) kept.push_back(std::move(ls[i]));
    ls = std::move(kept);
}

// Kernel choice, LDS budget, persistent grid, device tables and label of one launch: fixed here, by the launcher of its kind,
// and a program no kernel can run is refused whole (an eval then either runs every launch or none)
template <typename T>
int prepare_launch(Launch& L, const gaast_hip_program_s& prog) {
    const Plan& plan = prog.plan;
    Step& s = L.s;
    auto layout_of = [&](BufRef r) { return r.idx < 0 ? Layout() : plan.layout(r); };
    L.n = (s.kind == Step::PRODUCT_DENSE && s.dense.n) ? s.dense.n : plan.n;   // parity-pure products run in Cl(n - 1)
    L.domain = prog.domain.ptr;
    std::string kernel;
    const Layout la = layout_of(s.a), lb = layout_of(s.b);
    int st = GAAST_OK;
    switch (s.kind) {
    case Step::ZERO: break;   // (a memset: nothing to prepare)
    case Step::AXPY:
    case Step::FLIP:
    case Step::SUNARY: st = prepare_trivial<T>(L, kernel); break;
    case Step::PRODUCT_CSR: st = prepare_list<T>(L, la, lb, kernel); break;
    case Step::PRODUCT_DENSE: st = prepare_dense<T>(L, kernel); break;
    case Step::FUSED: st = prepare_fused<T>(L); break;
    case Step::EXPLOG: st = prepare_explog<T>(L); break;
    case Step::REDUCE_SCALE: st = prepare_reduce<T>(L, kernel); break;
    case Step::ELEMENTWISE: st = prepare_elementwise<T>(L, kernel); break;
    case Step::LINMAP: kernel = linmap_kernel_name(L.linmap->n, plan.dtype); break;
    case Step::EXPLOG_ADJ: st = prepare_explog_adj<T>(L, la, lb, kernel); break;
    case Step::DUAL: st = prepare_dual<T>(L, kernel); break;
    case Step::INVERSE: st = prepare_inverse<T>(L, kernel); break;
    case Step::GEXP:
    case Step::GEXP_ADJ: st = prepare_gexp<T>(L, kernel); break;
    case Step::GEXP_JVP:
    case Step::GEXP_ADJ2: st = prepare_gexp2<T>(L, kernel); break;
    case Step::GSQRT:
    case Step::GSQRT_ADJ:
    case Step::GSQRT_JVP: st = prepare_gsqrt<T>(L, kernel); break;
    case Step::GLOG:
    case Step::GLOG_ADJ:
    case Step::GLOG_JVP: st = prepare_glog<T>(L, kernel); break;
    case Step::GLOG_ADJ2: st = prepare_glog_adj2<T>(L, kernel); break;
    }
    if (st) return st;
    L.label = kernel.empty() ? s.name : s.name + " :: " + kernel;
    return GAAST_OK;
}
int prepare_launch(Launch& L, const gaast_hip_program_s& prog) {
    return prog.plan.dtype == GAAST_F32 ? prepare_launch<float>(L, prog) : prepare_launch<double>(L, prog);
}

// input slots some launch reads (the others may stay unbound)
void mark_used_slots(gaast_hip_program_s& prog) {
    Plan& plan = prog.plan;
    plan.slot_used.assign(plan.inputs.size(), 0);
    auto use = [&](BufRef r) {
        if (r.kind == BufKind::INPUT) plan.slot_used[size_t(r.idx)] = 1;
    };
    for (const Launch& L : prog.launches) for_each_read(L.s, use);
}

int upload_const_rows(gaast_hip_program_s& prog) {
    const Plan& plan = prog.plan;
    prog.const_rows.resize(plan.inputs.size());
    for (size_t i = 0; i < plan.inputs.size(); ++i)
        if (plan.inputs[i].is_const)
            if (int st = prog.const_rows[i].upload(plan.const_rows[i], plan.dtype)) return st;
    return GAAST_OK;
}

// mirrored: the program runs in the orthogonal basis of a Gram metric whose Q has determinant -1 (Plan::mirrored)
int program_create_impl(const gaast_program_desc* desc, gaast_hip_program_t* out, bool mirrored) {
    auto prog = std::make_unique<gaast_hip_program_s>();  // its destructor releases whatever a failure leaves behind
    if (int st = make_launches(*desc, false, mirrored, *prog)) return st;
    // a plan that can only run as the specialised kernel is rebuilt without run-time compilation if the compiler is not available
    uint32_t rebuild_flags = 0;
    bool small_reg_slab = false;
    for (int attempt = 0; attempt < 3 && compile_fused(*prog, desc->flags, &rebuild_flags, &small_reg_slab); ++attempt) {
        gaast_program_desc d2 = *desc;
        d2.flags |= rebuild_flags;
        if (int st = make_launches(d2, small_reg_slab, mirrored, *prog)) return st;
    }
    compile_chains(*prog, desc->flags);
    if (prog->plan.has_explog || prog->plan.has_inverse || prog->plan.has_gexp || prog->plan.has_gsqrt || prog->plan.has_glog)
        if (int st = prog->domain.upload(std::vector<unsigned long long>(1, 0))) return st;
    for (Launch& L : prog->launches)
        if (int st = prepare_launch(L, *prog)) return st;
    mark_used_slots(*prog);
    if (int st = upload_const_rows(*prog)) return st;
    *out = prog.release();
    return GAAST_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* gaast_hip_last_error(void) { return g_err.c_str(); }
const char* gaast_hip_version(void) { return "gaast-hip 0.2 (gfx950) kernels " GAAST_KERNELS_REV; }

int gaast_hip_init(const int* device_ids, int n_dev) {
    if (n_dev != 1 || !device_ids)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "one process drives one GPU: pass exactly one device id");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return set_err(GAAST_ERR_NO_DEVICE, "no HIP device visible");
    if (device_ids[0] < 0 || device_ids[0] >= count) return set_err(GAAST_ERR_INVALID_ARGUMENT, "device id out of range");
    HIP_TRY(hipSetDevice(device_ids[0]));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_ids[0]));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(GAAST_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only, found ") + prop.gcnArchName);
    g_num_cu = prop.multiProcessorCount;
    g_max_lds = prop.maxSharedMemoryPerMultiProcessor ? size_t(prop.maxSharedMemoryPerMultiProcessor) : size_t(160 * 1024);
    if (g_max_lds > 160 * 1024) g_max_lds = 160 * 1024;
    g_device = device_ids[0];
    g_stream = nullptr;
    // Load the library's code object NOW (HIP loads a fat binary lazily, at the first launch or attribute query of one of its
    // kernels): twice in round 3 a process that had compiled kernels through hiprtc first and launched its first statically
    // compiled kernel afterwards (tests/test_gpu_explog.py run alone: three hiprtc programs, then k_axpy_map / k_exp_log)
    // ended in a silent abort() inside that first launch; with the static code object resident before hiprtc is ever
    // initialised the order that preceded both aborts cannot occur.
    {
        hipFuncAttributes fa;
        HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_flip<double>)));
    }
    g_init = true;
    return GAAST_OK;
}

int gaast_hip_shutdown(void) {
    if (g_init) {
        (void)hipSetDevice(g_device);
        std::string err;
        (void)comm_destroy(g_comm, &err);
        for (hipEvent_t ev : g_events) (void)hipEventDestroy(ev);
        g_events.clear();
        if (g_comm_done) (void)hipEventDestroy(g_comm_done);
        g_comm_done = nullptr;
        if (g_comm_flag) (void)hipFree(g_comm_flag);
        g_comm_flag = nullptr;
        for (ReduceScratch& r : g_reduce_scratch) {
            (void)hipStreamSynchronize(r.stream);
            (void)hipFree(r.ptr);
        }
        g_reduce_scratch.clear();
    }
    g_init = false;
    return GAAST_OK;
}

int gaast_hip_set_stream(void* hip_stream) {
    g_stream = static_cast<hipStream_t>(hip_stream);
    return GAAST_OK;
}

int gaast_hip_synchronize(void) {
    if (int st = ensure_init()) return st;
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (g_comm.active()) HIP_TRY(hipStreamSynchronize(g_comm.stream));
    return GAAST_OK;
}

static int program_create_oriented(const gaast_program_desc* desc, gaast_hip_program_t* out, bool mirrored) {
    if (!desc || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    int st = program_create_impl(desc, out, mirrored);
    // a chain beyond the device's LDS: the unchained plan of the same program still runs -- rebuild without chains (as the
    // hiprtc-failure fallback does) instead of refusing the program
    if (st == kChainTooBig && !(desc->flags & GAAST_FLAG_DEBUG_NO_CHAIN)) {
        gaast_program_desc d2 = *desc;
        d2.flags |= GAAST_FLAG_DEBUG_NO_CHAIN;
        st = program_create_impl(&d2, out, mirrored);
    }
    return st == kChainTooBig ? GAAST_ERR_UNIMPLEMENTED : st;
}
int gaast_hip_program_create(const gaast_program_desc* desc, gaast_hip_program_t* out) { return program_create_oriented(desc, out, false); }

// ---- reverse mode -------------------------------------------------------------------------------------------------------
int gaast_hip_program_create_vjp(const gaast_program_desc* desc, int32_t wrt_slot, gaast_hip_program_t* out) {
    if (!desc || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    gaast_program_image_t img = nullptr;
    if (int st = gaast_program_vjp(desc, wrt_slot, &img)) return set_err(st, std::string("program_create_vjp: ") + gaast_expr_last_error());
    const int st = gaast_hip_program_create(gaast_program_image_desc(img), out);
    gaast_program_image_free(img);
    return st;
}

extern "C++" {
namespace {
int reduce_scratch(size_t bytes, void** ptr);
template <typename T>
int launch_sum_rows(gaast_hip_mv_t in, gaast_hip_mv_t out) {
    const int64_t B = in->batch, len = in->layout.row_len;
    if (len == 0) return GAAST_OK;
    const int64_t chunk = GAAST_SUM_ROWS_CHUNK, chunks = (B + chunk - 1) / chunk;
    const unsigned tiles = unsigned((len + kSumCols - 1) / kSumCols);
    T* dst = static_cast<T*>(out->ptr);
    if (chunks > 1) {
        void* scratch = nullptr;
        if (int st = reduce_scratch(size_t(chunks * len) * sizeof(T), &scratch)) return st;
        T* part = static_cast<T*>(scratch);
        hipLaunchKernelGGL(k_sum_rows<T>, dim3(unsigned(chunks), tiles), dim3(256), 0, g_stream,
                           static_cast<const T*>(in->ptr), in->row_stride, B, int(len), chunk, part, len);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sum_rows<T>, dim3(1u, tiles), dim3(256), 0, g_stream, static_cast<const T*>(part), len, chunks, int(len),
                           chunks, dst, len);
    } else {
        hipLaunchKernelGGL(k_sum_rows<T>, dim3(1u, tiles), dim3(256), 0, g_stream, static_cast<const T*>(in->ptr), in->row_stride, B,
                           int(len), chunk, dst, len);
    }
    HIP_TRY(hipGetLastError());
    return GAAST_OK;
}
}  // namespace
}  // extern "C++"

int gaast_hip_mv_sum_rows(gaast_hip_mv_t in, gaast_hip_mv_t out) {
    if (!in || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    if (out->batch != 1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "sum_rows: out must hold one row");
    if (in->batch < 1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "sum_rows: in holds no rows");
    if (in->layout.dim != out->layout.dim || in->layout.mask != out->layout.mask || in->dtype != out->dtype)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "sum_rows: in and out differ in dimension, grade mask or dtype");
    if (in->layout.row_len > (int64_t(1) << GAAST_MAX_DIM)) return set_err(GAAST_ERR_INVALID_ARGUMENT, "sum_rows: row too long");
    const size_t sz = dtype_size(in->dtype);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(in->ptr), b0 = reinterpret_cast<uintptr_t>(out->ptr);
    const uintptr_t a1 = a0 + size_t((in->batch - 1) * in->row_stride + in->layout.row_len) * sz, b1 = b0 + size_t(out->layout.row_len) * sz;
    if (a0 < b1 && b0 < a1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "sum_rows: in and out overlap");
    return in->dtype == GAAST_F32 ? launch_sum_rows<float>(in, out) : launch_sum_rows<double>(in, out);
}

// ---- linear maps of the vector space on graded rows (outermorphisms) --------------------------------------------------
int gaast_hip_linmap_create(int n, const double* matrix, int dtype, gaast_hip_linmap_t* out) {
    if (!matrix || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 1 || n > GAAST_MAX_DIM) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap: dimension out of range");
    if (dtype != GAAST_F32 && dtype != GAAST_F64) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap: unknown dtype");
    if (n > kLinmapMaxDim) return set_err(GAAST_ERR_UNIMPLEMENTED, "linmap: dimension above " + std::to_string(kLinmapMaxDim));
    for (int i = 0; i < n * n; ++i)
        if (!std::isfinite(matrix[i])) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap: matrix entry not finite");
    if (int st = ensure_init()) return st;
    auto m = std::make_unique<gaast_hip_linmap_s>();
    if (int st = linmap_build(n, matrix, dtype, m->dev)) return st;
    m->matrix.assign(matrix, matrix + n * n);
    *out = m.release();
    return GAAST_OK;
}

int gaast_hip_linmap_destroy(gaast_hip_linmap_t map) {
    if (!map) return GAAST_OK;
    if (g_init) (void)hipSetDevice(g_device);
    delete map;
    return GAAST_OK;
}

extern "C++" {
namespace {
// the argument checks and the launch of gaast_hip_linmap_apply, for the compounds `m` (those of M or of M^T)
int linmap_apply_impl(const LinmapDev& m, gaast_hip_mv_t in, gaast_hip_mv_t out) {
    if (in->layout.dim != m.n || out->layout.dim != m.n)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_apply: the rows' dimension differs from the map's");
    if (in->layout.mask != out->layout.mask) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_apply: in and out grade sets differ");
    if (in->batch != out->batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_apply: in and out batches differ");
    if (in->dtype != m.dtype || out->dtype != m.dtype) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_apply: dtype differs from the map's");
    const size_t sz = dtype_size(m.dtype);
    auto span = [&](gaast_hip_mv_t v, uintptr_t* lo, uintptr_t* hi) {
        *lo = reinterpret_cast<uintptr_t>(v->ptr);
        *hi = *lo + (v->batch > 0 ? size_t((v->batch - 1) * v->row_stride + v->layout.row_len) * sz : 0);
    };
    uintptr_t a0, a1, b0, b1;
    span(in, &a0, &a1);
    span(out, &b0, &b1);
    if (a0 < b1 && b0 < a1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_apply: in and out overlap");
    const Bound src{in->ptr, in->row_stride}, dst{out->ptr, out->row_stride};
    return m.dtype == GAAST_F32 ? launch_linmap<float>(m, in->layout, src, dst, in->batch)
                                : launch_linmap<double>(m, in->layout, src, dst, in->batch);
}

// the library's reduction scratch of the current stream (gaast_hip_mv_sum_rows' rules: one buffer per stream, grown after
// synchronising that stream only)
int reduce_scratch(size_t bytes, void** ptr) {
    ReduceScratch* sc = nullptr;
    for (ReduceScratch& r : g_reduce_scratch)
        if (r.stream == g_stream) sc = &r;
    if (!sc) {
        g_reduce_scratch.push_back(ReduceScratch{g_stream, nullptr, 0});
        sc = &g_reduce_scratch.back();
    }
    if (bytes > sc->bytes) {
        if (sc->ptr) {
            HIP_TRY(hipStreamSynchronize(g_stream));   // an earlier reduction on this stream may still read it
            HIP_TRY(hipFree(sc->ptr));
            sc->ptr = nullptr;
            sc->bytes = 0;
        }
        HIP_TRY(hipMalloc(&sc->ptr, bytes));
        sc->bytes = bytes;
    }
    *ptr = sc->ptr;
    return GAAST_OK;
}

constexpr int kLinmapVjpMaxDim = 8;   // W has C(2n,n) entries; a term word indexes W and the compounds in 14 bits each
static_assert(kOuterChunk == GAAST_SUM_ROWS_CHUNK, "the first level of the outer-sum tree is gaast_hip_mv_sum_rows' chunk");

// the term table of dL/dM for rows holding the grades of `mask`: W_k at the offset k_linmap_outer_sum writes it, C_{k-1} where the
// map holds it, stably sorted by target (i, j) -- so a target's terms stay ordered by grade, I, J
int linmap_vjp_table(gaast_hip_linmap_s& map, uint64_t mask, const gaast_hip_linmap_s::VjpTable** out) {
    auto it = map.vjp_tables.find(mask);
    if (it == map.vjp_tables.end()) {
        const int n = map.dev.n;
        const BladeTable bt(n);
        std::vector<std::vector<uint32_t>> per_target(size_t(n * n));
        std::vector<CompoundVjpTerm> terms;
        uint32_t woff = 0;
        for (int k = 1; k <= n; ++k) {
            if (!((mask >> k) & 1ULL)) continue;
            compound_vjp_terms(bt, k, terms);
            for (const CompoundVjpTerm& e : terms) {
                const uint32_t wi = woff + e.w, ci = uint32_t(map.dev.moff[size_t(k - 1)]) + e.minor;
                if ((wi | ci) >> kContractIndexBits) return set_err(GAAST_ERR_UNIMPLEMENTED, "linmap_matrix_vjp: term index out of range");
                per_target[e.target].push_back(wi | ci << kContractIndexBits | uint32_t(e.negative) << (2 * kContractIndexBits));
            }
            woff += bt.grade_dim[size_t(k)] * bt.grade_dim[size_t(k)];
        }
        std::vector<uint32_t> words, row_start(size_t(n * n + 1), 0);
        for (size_t t = 0; t < per_target.size(); ++t) {
            words.insert(words.end(), per_target[t].begin(), per_target[t].end());
            row_start[t + 1] = uint32_t(words.size());
        }
        gaast_hip_linmap_s::VjpTable tab;
        if (int st = tab.terms.upload(std::move(words))) return st;
        if (int st = tab.row_start.upload(std::move(row_start))) return st;
        it = map.vjp_tables.emplace(mask, std::move(tab)).first;
    }
    *out = &it->second;
    return GAAST_OK;
}

template <typename T>
int launch_linmap_matrix_vjp(gaast_hip_linmap_s& map, gaast_hip_mv_t in, gaast_hip_mv_t cot, void* dm) {
    const LinmapDev& m = map.dev;
    const Layout& l = in->layout;
    const gaast_hip_linmap_s::VjpTable* tab = nullptr;
    if (int st = linmap_vjp_table(map, l.mask, &tab)) return st;
    OuterSumArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.g = static_cast<const T*>(cot->ptr);
    p.x = static_cast<const T*>(in->ptr);
    p.g_stride = cot->row_stride;
    p.x_stride = in->row_stride;
    p.batch = in->batch;
    for (int k = 1; k <= m.n; ++k) {
        if (!((l.mask >> k) & 1ULL)) continue;
        const int len = int(n_choose_k(uint64_t(m.n), uint64_t(k))), tl = (len + 15) / 16;
        const int g = p.n_grades++;
        p.goff[g] = int(l.offset(k));
        p.glen[g] = len;
        p.woff[g] = p.w_total;
        p.w_total += len * len;
        p.tile0[g + 1] = p.tile0[g] + tl * tl;
    }
    p.n_tiles = p.tile0[p.n_grades];
    const int64_t chunks = (in->batch + kOuterChunk - 1) / kOuterChunk;
    T* w = nullptr;
    if (p.n_tiles > 0) {
        void* sc = nullptr;   // W, then (more than one chunk) the chunk partials
        if (int st = reduce_scratch(size_t(chunks > 1 ? chunks + 1 : 1) * size_t(p.w_total) * sizeof(T), &sc)) return st;
        w = static_cast<T*>(sc);
        p.out = chunks > 1 ? w + p.w_total : w;
        hipLaunchKernelGGL(k_linmap_outer_sum<T>, dim3(unsigned((p.n_tiles + kOuterWaves - 1) / kOuterWaves), unsigned(chunks)),
                           dim3(64 * kOuterWaves), 0, g_stream, p);
        HIP_TRY(hipGetLastError());
        if (chunks > 1) {
            const unsigned tiles = unsigned((p.w_total + kSumCols - 1) / kSumCols);
            hipLaunchKernelGGL(k_sum_rows<T>, dim3(1u, tiles), dim3(256), 0, g_stream, static_cast<const T*>(p.out), int64_t(p.w_total),
                               chunks, p.w_total, chunks, w, int64_t(p.w_total));
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_linmap_minor_contract<T>, dim3(unsigned(m.n * m.n)), dim3(kContractThreads), 0, g_stream, static_cast<const T*>(w),
                       m.mats.as<T>(), tab->terms.template as<uint32_t>(), tab->row_start.template as<uint32_t>(), static_cast<T*>(dm));
    HIP_TRY(hipGetLastError());
    return GAAST_OK;
}
}  // namespace
}  // extern "C++"

int gaast_hip_linmap_apply(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t out) {
    if (!map || !in || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    return linmap_apply_impl(map->dev, in, out);
}

int gaast_hip_linmap_apply_transposed(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t out) {
    if (!map || !in || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    if (!map->transposed) {
        const int n = map->dev.n;
        std::vector<double> mt(size_t(n * n));
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) mt[size_t(i * n + j)] = map->matrix[size_t(j * n + i)];
        auto t = std::make_unique<LinmapDev>();
        if (int st = linmap_build(n, mt.data(), map->dev.dtype, *t)) return st;
        map->transposed = std::move(t);
    }
    return linmap_apply_impl(*map->transposed, in, out);
}

int gaast_hip_linmap_matrix_vjp(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t cotangent, void* dmatrix_dev) {
    if (!map || !in || !cotangent || !dmatrix_dev) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    const LinmapDev& m = map->dev;
    if (m.n > kLinmapVjpMaxDim)
        return set_err(GAAST_ERR_UNIMPLEMENTED, "linmap_matrix_vjp: dimension above " + std::to_string(kLinmapVjpMaxDim));
    if (in->layout.dim != m.n || cotangent->layout.dim != m.n)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: the rows' dimension differs from the map's");
    if (in->layout.mask != cotangent->layout.mask) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: in and cotangent grade sets differ");
    if (in->batch != cotangent->batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: in and cotangent batches differ");
    if (in->batch < 1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: the rows hold no items");
    if ((in->batch + kOuterChunk - 1) / kOuterChunk > 65535) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: more than 65535 chunks of items");
    if (in->dtype != m.dtype || cotangent->dtype != m.dtype) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: dtype differs from the map's");
    const size_t sz = dtype_size(m.dtype);
    if (reinterpret_cast<uintptr_t>(dmatrix_dev) % sz) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: dmatrix_dev is not element-aligned");
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dmatrix_dev), d1 = d0 + size_t(m.n * m.n) * sz;
    for (gaast_hip_mv_t v : {in, cotangent}) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(v->ptr), a1 = a0 + size_t((v->batch - 1) * v->row_stride + v->layout.row_len) * sz;
        if (a0 < d1 && d0 < a1) return set_err(GAAST_ERR_INVALID_ARGUMENT, "linmap_matrix_vjp: dmatrix_dev overlaps the rows");
    }
    return m.dtype == GAAST_F32 ? launch_linmap_matrix_vjp<float>(*map, in, cotangent, dmatrix_dev)
                                : launch_linmap_matrix_vjp<double>(*map, in, cotangent, dmatrix_dev);
}

// A program specialised for the orthogonal basis f_j = sum_i Q_ij e_i, evaluated on rows in the caller's basis e: inputs move into f
// through C_k(Q^T), the result back through C_k(Q) (LINMAP steps around the program's own plan).  Q == I exactly: the plain program.
int gaast_hip_program_create_in_basis(const gaast_program_desc* desc, const double* basis, gaast_hip_program_t* out) {
    if (!desc || !basis || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    const int n = desc->vec_space_dim;
    if (n < 1 || n > GAAST_MAX_DIM) return set_err(GAAST_ERR_INVALID_ARGUMENT, "program_create_in_basis: dimension out of range");
    bool identity = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double q = basis[i * n + j];
            if (!std::isfinite(q)) return set_err(GAAST_ERR_INVALID_ARGUMENT, "program_create_in_basis: basis entry not finite");
            identity = identity && q == (i == j ? 1.0 : 0.0);
            double qtq = 0.0;   // (Q^T Q)_ij
            for (int k = 0; k < n; ++k) qtq += basis[k * n + i] * basis[k * n + j];
            if (std::fabs(qtq - (i == j ? 1.0 : 0.0)) > 1e-12)
                return set_err(GAAST_ERR_INVALID_ARGUMENT, "program_create_in_basis: the basis is not orthogonal (|Q^T Q - I| > 1e-12)");
        }
    if (identity) return gaast_hip_program_create(desc, out);
    if (int st = ensure_init()) return st;
    if (n > kLinmapMaxDim)
        return set_err(GAAST_ERR_UNIMPLEMENTED, "program_create_in_basis: dimension above " + std::to_string(kLinmapMaxDim));
    std::vector<double> qt(size_t(n * n));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) qt[size_t(i * n + j)] = basis[j * n + i];
    auto to_f = std::make_unique<LinmapDev>(), to_e = std::make_unique<LinmapDev>();
    std::vector<double> c_in;   // C_k(Q^T) in double: the constant inputs move on the host
    if (int st = linmap_build(n, qt.data(), desc->dtype, *to_f, &c_in)) return st;
    if (int st = linmap_build(n, basis, desc->dtype, *to_e)) return st;
    // constant rows into f; a row of another dimension can only be a scalar
    gaast_program_desc d2 = *desc;
    std::vector<gaast_input_desc> ins(desc->inputs, desc->inputs + (desc->n_inputs > 0 ? desc->n_inputs : 0));
    std::vector<std::vector<double>> rows(ins.size());
    for (size_t i = 0; i < ins.size(); ++i) {
        const gaast_input_desc& in = ins[i];
        if (!(in.grade_mask & ~1ULL)) continue;
        if (in.storage_dim != n)
            return set_err(GAAST_ERR_UNIMPLEMENTED, "program_create_in_basis: input slot " + std::to_string(i) + " has grades above 0 in another dimension");
        if (!in.is_const || !in.const_row) continue;
        const Layout l = make_layout(n, in.grade_mask);
        rows[i].assign(in.const_row, in.const_row + l.row_len);
        for (int k = 1; k <= n; ++k) {
            const int64_t off = l.offset(k);
            if (off < 0) continue;
            const int64_t d = l.grade_len(k);
            for (int64_t r = 0; r < d; ++r) {
                double acc = 0.0;
                for (int64_t c = 0; c < d; ++c) acc += c_in[size_t(to_f->moff[size_t(k)] + r * d + c)] * in.const_row[off + c];
                rows[i][size_t(off + r)] = acc;
            }
        }
        ins[i].const_row = rows[i].data();
    }
    d2.inputs = ins.empty() ? nullptr : ins.data();
    // the complement of the caller's basis is det(Q) = +-1 times the one of the orthogonal basis (gaast_hip.h: GAAST_OP_DUAL)
    gaast_hip_program_t prog = nullptr;
    if (int st = program_create_oriented(&d2, &prog, basis_is_mirrored(n, basis))) return st;
    std::unique_ptr<gaast_hip_program_s> owner(prog);
    Plan& plan = prog->plan;
    if (plan.out_layout.dim != n && (plan.out_layout.mask & ~1ULL))
        return set_err(GAAST_ERR_UNIMPLEMENTED, "program_create_in_basis: the result has grades above 0 in another dimension");
    // LINMAP launches: every batched input a launch reads, with grades above 0, into a node buffer of its own; the root back into out
    std::vector<Launch> launches;
    plan.basis_slot_buf.assign(plan.inputs.size(), -1);
    auto add_linmap = [&](const LinmapDev* m, BufRef res, BufRef a, const std::string& name) -> int {
        Launch L;
        L.s.kind = Step::LINMAP;
        L.s.res = res;
        L.s.a = a;
        L.s.name = name;
        L.linmap = m;
        if (int st = prepare_launch(L, *prog)) return st;
        launches.push_back(std::move(L));
        return GAAST_OK;
    };
    for (size_t i = 0; i < plan.inputs.size(); ++i) {
        if (plan.inputs[i].is_const || !plan.slot_used[i] || !(plan.inputs[i].grade_mask & ~1ULL)) continue;
        const int buf = int(plan.node_buffers.size());
        plan.node_buffers.push_back(plan.input_layouts[i]);
        if (!plan.node_dead.empty()) plan.node_dead.push_back(0);
        plan.basis_slot_buf[i] = buf;
        if (int st = add_linmap(to_f.get(), BufRef{BufKind::NODE, buf}, BufRef{BufKind::INPUT, int(i)},
                                "linmap[input " + std::to_string(i) + " -> orthogonal basis]"))
            return st;
    }
    for (Launch& L : prog->launches) launches.push_back(std::move(L));
    if (plan.out_layout.mask & ~1ULL) {
        plan.basis_out_buf = int(plan.node_buffers.size());
        plan.node_buffers.push_back(plan.out_layout);
        if (!plan.node_dead.empty()) plan.node_dead.push_back(0);
        if (int st = add_linmap(to_e.get(), BufRef{BufKind::OUT, -1}, BufRef{BufKind::NODE, plan.basis_out_buf}, "linmap[result -> caller's basis]"))
            return st;
    }
    prog->launches = std::move(launches);
    prog->basis_in = std::move(to_f);
    prog->basis_out = std::move(to_e);
    prog->scratch_batch = 0;   // the node buffers are re-allocated at the next eval
    *out = owner.release();
    return GAAST_OK;
}

// y_e = C(Q) F(C(Q^T) x_e) with orthogonal C_k(Q): the VJP of the in-basis program is the in-basis version of F's VJP program
int gaast_hip_program_create_vjp_in_basis(const gaast_program_desc* desc, const double* basis, int32_t wrt_slot, gaast_hip_program_t* out) {
    if (!desc || !basis || !out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    gaast_program_image_t img = nullptr;
    if (int st = gaast_program_vjp(desc, wrt_slot, &img)) return set_err(st, std::string("program_create_vjp_in_basis: ") + gaast_expr_last_error());
    gaast_hip_program_t prog = nullptr;
    const int st = gaast_hip_program_create_in_basis(gaast_program_image_desc(img), basis, &prog);
    gaast_program_image_free(img);
    if (st == GAAST_OK) *out = prog;
    return st;
}

int gaast_hip_program_destroy(gaast_hip_program_t prog) {
    if (!prog) return GAAST_OK;
    if (g_init) {
        (void)hipSetDevice(g_device);
        // launches of this program may still be in flight: a hiprtc module must not be unloaded (nor a table freed) under them
        (void)hipStreamSynchronize(g_stream);
    }
    delete prog;
    return GAAST_OK;
}

int gaast_hip_jit_cache_set_dir(const char* path) {
    JitCache& c = jit_cache();
    std::lock_guard<std::mutex> lock(c.mutex);
    c.dir.clear();
    if (!path || !*path) return GAAST_OK;
    if (!jitcache::prepare_dir(path))
        return set_err(GAAST_ERR_INVALID_ARGUMENT, std::string("jit_cache_set_dir: cannot create or is not a directory: ") + path);
    c.dir = path;
    return GAAST_OK;
}

int gaast_hip_jit_cache_stats(int64_t* out, int n) {
    JitCache& c = jit_cache();
    for (int i = 0; out && i < n && i < JIT_N_COUNTERS; ++i) out[i] = c.counters[i].load();
    return JIT_N_COUNTERS;
}

int gaast_hip_program_domain_errors(gaast_hip_program_t prog, int64_t* count) {
    if (!prog || !count) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    *count = 0;
    if (!prog->domain.ptr) return GAAST_OK;
    HIP_TRY(hipStreamSynchronize(g_stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, prog->domain.ptr, sizeof(v), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(prog->domain.ptr, 0, sizeof(v)));
    *count = int64_t(v);
    return GAAST_OK;
}

const char* gaast_hip_program_jit_source(gaast_hip_program_t prog) {
    return prog ? prog->plan.jit_source_kept.c_str() : "";
}

int gaast_hip_program_output_info(gaast_hip_program_t prog, uint64_t* grade_mask, int64_t* row_len) {
    if (!prog) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null program");
    if (grade_mask) *grade_mask = prog->plan.out_layout.mask;
    if (row_len) *row_len = prog->plan.out_layout.row_len;
    return GAAST_OK;
}

int gaast_hip_program_num_launches(gaast_hip_program_t prog) { return prog ? int(prog->launches.size()) : 0; }
const char* gaast_hip_program_launch_name(gaast_hip_program_t prog, int i) {
    if (!prog || i < 0 || i >= int(prog->launches.size())) return "";
    return prog->launches[size_t(i)].label.c_str();
}
int gaast_hip_program_launch_variant(gaast_hip_program_t prog, int i) {
    if (!prog || i < 0 || i >= int(prog->launches.size())) return -1;
    return prog->launches[size_t(i)].variant;
}

int gaast_hip_mv_alloc(int dim, uint64_t grade_mask, int64_t batch, int dtype, gaast_hip_mv_t* out) {
    if (!out || dim < 0 || dim > GAAST_MAX_DIM || batch < 0 || (dtype != GAAST_F64 && dtype != GAAST_F32))
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "bad mv_alloc argument");
    if (int st = ensure_init()) return st;
    return mv_alloc_impl(dim, grade_mask, batch, dtype, out);
}

int gaast_hip_mv_wrap(void* device_ptr, int dim, uint64_t grade_mask, int64_t batch, int dtype,
                      int64_t row_stride, gaast_hip_mv_t* out) {
    if (!out || dim < 0 || dim > GAAST_MAX_DIM || batch < 0 || (dtype != GAAST_F64 && dtype != GAAST_F32))
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "bad mv_wrap argument");
    // every kernel addresses the rows as elements: a base that is not a multiple of the element size cannot be one
    if (reinterpret_cast<uintptr_t>(device_ptr) % dtype_size(dtype) != 0)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "mv_wrap: device_ptr is not aligned to the element size");
    auto* m = new gaast_hip_mv_s;
    m->layout = make_layout(dim, grade_mask);
    if (row_stride < m->layout.row_len && !(batch <= 1)) {
        delete m;
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "row_stride shorter than the row");
    }
    // a single row has no stride to speak of: keep the 2-D copies / memsets well-formed (pitch >= width)
    if (batch <= 1 && row_stride < m->layout.row_len) row_stride = m->layout.row_len;
    m->batch = batch;
    m->dtype = dtype;
    m->row_stride = row_stride;
    m->ptr = device_ptr;
    m->owns = false;
    *out = m;
    return GAAST_OK;
}

int gaast_hip_mv_free(gaast_hip_mv_t mv) {
    mv_free_impl(mv);
    return GAAST_OK;
}

int gaast_hip_mv_info(gaast_hip_mv_t mv, int* dim, uint64_t* grade_mask, int64_t* batch, int* dtype,
                      int64_t* row_len, int64_t* row_stride, void** device_ptr) {
    if (!mv) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null mv");
    if (dim) *dim = mv->layout.dim;
    if (grade_mask) *grade_mask = mv->layout.mask;
    if (batch) *batch = mv->batch;
    if (dtype) *dtype = mv->dtype;
    if (row_len) *row_len = mv->layout.row_len;
    if (row_stride) *row_stride = mv->row_stride;
    if (device_ptr) *device_ptr = mv->ptr;
    return GAAST_OK;
}

static int mv_copy_grade(gaast_hip_mv_t mv, int grade, void* host, int64_t count, bool upload) {
    if (!mv || !host) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    if (grade < 0 || grade > 63 || !((mv->layout.mask >> grade) & 1ULL))
        return set_err(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(grade) + " absent from this multivector");
    const int64_t glen = mv->layout.grade_len(grade);
    if (count != glen * mv->batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "count must be C(dim,k) * batch");
    if (count == 0) return GAAST_OK;
    const size_t sz = dtype_size(mv->dtype);
    char* dev = static_cast<char*>(mv->ptr) + size_t(mv->layout.offset(grade)) * sz;
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (upload)
        HIP_TRY(hipMemcpy2D(dev, size_t(mv->row_stride) * sz, host, size_t(glen) * sz, size_t(glen) * sz,
                            size_t(mv->batch), hipMemcpyHostToDevice));
    else
        HIP_TRY(hipMemcpy2D(host, size_t(glen) * sz, dev, size_t(mv->row_stride) * sz, size_t(glen) * sz,
                            size_t(mv->batch), hipMemcpyDeviceToHost));
    return GAAST_OK;
}

int gaast_hip_mv_upload(gaast_hip_mv_t mv, int grade, const void* host, int64_t count) {
    return mv_copy_grade(mv, grade, const_cast<void*>(host), count, true);
}
int gaast_hip_mv_download(gaast_hip_mv_t mv, int grade, void* host, int64_t count) {
    return mv_copy_grade(mv, grade, host, count, false);
}

static int mv_copy_rows(gaast_hip_mv_t mv, void* host, int64_t count, bool upload) {
    if (!mv || (!host && count)) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    const int64_t rl = mv->layout.row_len;
    if (count != rl * mv->batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "count must be row_len * batch");
    if (count == 0) return GAAST_OK;
    const size_t sz = dtype_size(mv->dtype);
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (upload)
        HIP_TRY(hipMemcpy2D(mv->ptr, size_t(mv->row_stride) * sz, host, size_t(rl) * sz, size_t(rl) * sz,
                            size_t(mv->batch), hipMemcpyHostToDevice));
    else
        HIP_TRY(hipMemcpy2D(host, size_t(rl) * sz, mv->ptr, size_t(mv->row_stride) * sz, size_t(rl) * sz,
                            size_t(mv->batch), hipMemcpyDeviceToHost));
    return GAAST_OK;
}

int gaast_hip_mv_upload_rows(gaast_hip_mv_t mv, const void* host, int64_t count) {
    return mv_copy_rows(mv, const_cast<void*>(host), count, true);
}
int gaast_hip_mv_download_rows(gaast_hip_mv_t mv, void* host, int64_t count) {
    return mv_copy_rows(mv, host, count, false);
}

int gaast_hip_mv_zero(gaast_hip_mv_t mv) {
    if (!mv) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null mv");
    if (int st = ensure_init()) return st;
    const size_t sz = dtype_size(mv->dtype);
    if (mv->batch && mv->layout.row_len)
        HIP_TRY(hipMemset2DAsync(mv->ptr, size_t(mv->row_stride) * sz, 0, size_t(mv->layout.row_len) * sz,
                                 size_t(mv->batch), g_stream));
    return GAAST_OK;
}

}  // extern "C"

namespace {

// argument checks of an eval + the (pointer, stride) of every bound input, for items [0, batch)
int bind_eval(gaast_hip_program_t prog, const gaast_hip_mv_t* inputs, int n_inputs, int64_t batch, gaast_hip_mv_t out,
              std::vector<Bound>& in_bound) {
    if (!prog || !out || batch < 0) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    Plan& plan = prog->plan;
    if (plan.error != GAAST_OK) return set_err(plan.error, plan.error_msg);  // the reference panics here
    if (n_inputs < 0 || (n_inputs && !inputs)) return set_err(GAAST_ERR_INVALID_ARGUMENT, "bad inputs");
    in_bound.assign(plan.inputs.size(), Bound{nullptr, 0});
    for (size_t i = 0; i < plan.inputs.size(); ++i) {
        const Layout& want = plan.input_layouts[i];
        if (plan.inputs[i].is_const) {   // one row, shared by every item
            in_bound[i] = Bound{prog->const_rows[i].ptr, batch != 1 ? 0 : want.row_len};
            continue;
        }
        gaast_hip_mv_t m = int(i) < n_inputs ? inputs[i] : nullptr;
        if (!m) {
            // slots no launch reads may stay unbound
            if (plan.slot_used[i]) return set_err(GAAST_ERR_INVALID_ARGUMENT, "input slot " + std::to_string(i) + " is not bound");
            continue;
        }
        if (m->layout.mask != want.mask || m->layout.dim != want.dim)
            return set_err(GAAST_ERR_INVALID_ARGUMENT, "input slot " + std::to_string(i) + ": grade set / dimension differ from the program's");
        if (m->dtype != plan.dtype) return set_err(GAAST_ERR_INVALID_ARGUMENT, "input dtype differs from the program's");
        if (m->batch != batch && m->batch != 1)
            return set_err(GAAST_ERR_INVALID_ARGUMENT, "input batch must equal the eval batch or be 1 (shared)");
        in_bound[i] = Bound{m->ptr, (m->batch == 1 && batch != 1) ? 0 : m->row_stride};
    }
    if (out->layout.mask != plan.out_layout.mask || out->layout.dim != plan.out_layout.dim)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "output grade set / dimension differ from the root's");
    if (out->dtype != plan.dtype || out->batch != batch)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "output dtype / batch mismatch");
    return GAAST_OK;
}

// One launch of an evaluation over `batch` items, by the launcher of its kind
template <typename T>
int run_launch(const Launch& L, const Operands& o, int64_t batch) {
    int variant = 0, st = GAAST_OK;   // (0: a launcher with one kernel)
    switch (L.s.kind) {
    case Step::ZERO:
        if (o.lres.row_len) HIP_TRY(hipMemset2DAsync(o.res.ptr, size_t(o.res.stride) * sizeof(T), 0, size_t(o.lres.row_len) * sizeof(T), size_t(batch), g_stream));
        break;
    case Step::AXPY:
    case Step::FLIP:
    case Step::SUNARY: st = run_trivial<T>(L, o, batch); break;
    case Step::PRODUCT_CSR: st = run_list<T>(L, o, batch, &variant); break;
    case Step::PRODUCT_DENSE: st = run_dense<T>(L, o, batch, &variant); break;
    case Step::FUSED: st = run_fused<T>(L, o, batch, &variant); break;
    case Step::EXPLOG: st = run_explog<T>(L, o, batch); break;
    case Step::REDUCE_SCALE: st = run_reduce<T>(L, o, batch, &variant); break;
    case Step::ELEMENTWISE: st = run_elementwise<T>(L, o, batch); break;
    case Step::LINMAP: st = run_linmap<T>(L, o, batch); break;
    case Step::EXPLOG_ADJ: st = run_explog_adj<T>(L, o, batch); break;
    case Step::DUAL: st = run_dual<T>(L, o, batch); break;
    case Step::INVERSE: st = run_inverse<T>(L, o, batch); break;
    case Step::GEXP:
    case Step::GEXP_ADJ: st = run_gexp<T>(L, o, batch); break;
    case Step::GEXP_JVP:
    case Step::GEXP_ADJ2: st = run_gexp2<T>(L, o, batch); break;
    case Step::GSQRT:
    case Step::GSQRT_ADJ:
    case Step::GSQRT_JVP: st = run_gsqrt<T>(L, o, batch); break;
    case Step::GLOG:
    case Step::GLOG_ADJ:
    case Step::GLOG_JVP: st = run_glog<T>(L, o, batch); break;
    case Step::GLOG_ADJ2: st = run_glog_adj2<T>(L, o, batch); break;
    }
    L.variant = variant;
    return st;
}

template <typename T>
int run_launches(gaast_hip_program_t prog, const std::vector<Bound>& in_bound, gaast_hip_mv_t out, int64_t first, int64_t count) {
    const Plan& plan = prog->plan;
    auto shifted = [&](Bound b) {
        if (b.ptr && first) b.ptr = static_cast<char*>(b.ptr) + size_t(first) * size_t(b.stride) * sizeof(T);
        return b;
    };
    EvalRows rows;
    rows.prog = prog;
    rows.out_layout = &out->layout;
    rows.callers.resize(in_bound.size());
    for (size_t i = 0; i < in_bound.size(); ++i) rows.callers[i] = shifted(in_bound[i]);
    rows.out_callers = shifted(Bound{out->ptr, out->row_stride});

    // cache buffers of the product operands (the per-eval HashMap<NodeId, R> of eval.rs:16)
    if (prog->scratch_batch < count || prog->scratch.size() != plan.node_buffers.size()) {
        if (!prog->scratch.empty()) HIP_TRY(hipStreamSynchronize(g_stream));  // launches may still read the old ones
        prog->scratch.clear();
        for (size_t bi = 0; bi < plan.node_buffers.size(); ++bi) {
            const Layout& l = plan.node_buffers[bi];
            gaast_hip_mv_t m = nullptr;
            // a cache buffer a chained product made unnecessary is never allocated
            const bool dead = bi < plan.node_dead.size() && plan.node_dead[bi];
            if (int st = mv_alloc_impl(l.dim, l.mask, dead ? 0 : count, plan.dtype, &m)) return st;
            prog->scratch.emplace_back(m);
        }
        prog->scratch_batch = count;
    }

    // a program in a non-orthonormal basis: every step but LINMAP reads the inputs' rows moved into the orthogonal basis (a shared
    // input: one row, broadcast) and writes the root into a node buffer that the last LINMAP step moves back into `out`
    rows.moved = rows.callers;
    rows.out_moved = rows.out_callers;
    for (size_t i = 0; i < plan.basis_slot_buf.size(); ++i) {
        if (plan.basis_slot_buf[i] < 0 || !rows.callers[i].ptr) continue;
        gaast_hip_mv_t m = prog->scratch[size_t(plan.basis_slot_buf[i])].get();
        rows.moved[i] = Bound{m->ptr, rows.callers[i].stride == 0 ? 0 : m->row_stride};
    }
    if (plan.basis_out_buf >= 0) {
        gaast_hip_mv_t m = prog->scratch[size_t(plan.basis_out_buf)].get();
        rows.out_moved = Bound{m->ptr, m->row_stride};
    }
    for (const Launch& L : prog->launches) {
        const Step& s = L.s;
        const bool callers_rows = s.kind == Step::LINMAP;   // the caller's rows in, the caller's rows out
        Operands o;
        o.rows = &rows;
        Layout unused;
        auto at = [&](BufRef r, Layout* lay) {   // (an operand the step does not have stays null)
            return r.idx >= 0 ? rows.at(r, lay, callers_rows) : Bound{nullptr, 0};
        };
        o.res = rows.at(s.res, &o.lres, callers_rows);
        o.a = at(s.a, &o.la);
        o.b = at(s.b, &o.lb);
        o.c = at(s.c, &unused);
        o.pre_a = at(s.pre.a, &unused);
        o.pre_b = at(s.pre.b, &unused);
        o.scaled_row = at(s.reduce.x, &unused);
        o.init = at(s.cj.init_src, &unused);
        if (int st = run_launch<T>(L, o, count)) return st;
    }
    return GAAST_OK;
}

// the launches of one evaluation over items [first, first + count) of the bound buffers
int eval_range(gaast_hip_program_t prog, const std::vector<Bound>& in_bound, gaast_hip_mv_t out, int64_t first, int64_t count) {
    const Plan& plan = prog->plan;
    if (plan.flags & GAAST_FLAG_DEBUG_FAIL_EVAL) return set_err(GAAST_ERR_HIP, "injected evaluation failure (GAAST_FLAG_DEBUG_FAIL_EVAL)");
    if (count == 0) return GAAST_OK;
    return plan.dtype == GAAST_F32 ? run_launches<float>(prog, in_bound, out, first, count) : run_launches<double>(prog, in_bound, out, first, count);
}

int rccl_err(const std::string& msg) { return set_err(GAAST_ERR_RCCL, msg); }

// items [lo, hi) of chunk c when `count` items are cut into n_chunks contiguous chunks
void chunk_span(int64_t count, int n_chunks, int c, int64_t* lo, int64_t* hi) {
    const int64_t per = (count + n_chunks - 1) / n_chunks;
    *lo = std::min<int64_t>(int64_t(c) * per, count);
    *hi = std::min<int64_t>(*lo + per, count);
}

// chunk c of every rank's rows travels to root on the communicator's stream (the caller has made that stream
// wait for the chunk's compute)
int gather_chunk(gaast_hip_mv_t local, gaast_hip_mv_t gathered, const int64_t* counts, int root, int n_chunks, int c) {
    std::string err;
    const size_t sz = dtype_size(local->dtype);
    const size_t row = size_t(local->layout.row_len);
    if (g_comm.rank != root) {
        int64_t lo, hi;
        chunk_span(counts[g_comm.rank], n_chunks, c, &lo, &hi);
        if (hi > lo && row)
            if (comm_send(g_comm, static_cast<const char*>(local->ptr) + size_t(lo) * row * sz, size_t(hi - lo) * row, int(sz),
                          root, &err))
                return rccl_err(err);
        return GAAST_OK;
    }
    // root: one receive per peer, grouped, so that the transfers of all xGMI links are in flight together
    if (comm_group_start(&err)) return rccl_err(err);
    int64_t first = 0;
    int failed = 0;
    for (int r = 0; r < g_comm.world; ++r) {
        int64_t lo, hi;
        chunk_span(counts[r], n_chunks, c, &lo, &hi);
        if (r != root && hi > lo && row && !failed)
            failed = comm_recv(g_comm, static_cast<char*>(gathered->ptr) + size_t(first + lo) * row * sz, size_t(hi - lo) * row,
                               int(sz), r, &err);
        first += counts[r];
    }
    std::string err2;
    if (comm_group_end(&err2) && !failed) return rccl_err(err2);
    if (failed) return rccl_err(err);
    // the root's own rows: a device copy, unless `out` already is that part of `gathered`
    int64_t lo, hi, first_root = 0;
    for (int r = 0; r < root; ++r) first_root += counts[r];
    chunk_span(counts[root], n_chunks, c, &lo, &hi);
    char* dst = static_cast<char*>(gathered->ptr) + size_t(first_root + lo) * row * sz;
    const char* src = static_cast<const char*>(local->ptr) + size_t(lo) * row * sz;
    if (hi > lo && row && dst != src)
        HIP_TRY(hipMemcpyAsync(dst, src, size_t(hi - lo) * row * sz, hipMemcpyDeviceToDevice, g_comm.stream));
    return GAAST_OK;
}

int check_gather_args(gaast_hip_mv_t local, gaast_hip_mv_t gathered, const int64_t* counts, int root) {
    if (!g_comm.active()) return rccl_err("no communicator: call gaast_hip_comm_init first");
    if (!local || !counts || root < 0 || root >= g_comm.world) return set_err(GAAST_ERR_INVALID_ARGUMENT, "bad gather argument");
    int64_t total = 0;
    for (int r = 0; r < g_comm.world; ++r) {
        if (counts[r] < 0) return set_err(GAAST_ERR_INVALID_ARGUMENT, "negative row count");
        total += counts[r];
    }
    if (counts[g_comm.rank] > local->batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "counts[rank] exceeds the local batch");
    if (local->row_stride != local->layout.row_len && local->batch > 1)
        return set_err(GAAST_ERR_INVALID_ARGUMENT, "gather needs contiguous rows (row_stride == row_len)");
    if (g_comm.rank == root) {
        if (!gathered) return set_err(GAAST_ERR_INVALID_ARGUMENT, "root needs a destination");
        if (gathered->layout.mask != local->layout.mask || gathered->layout.dim != local->layout.dim || gathered->dtype != local->dtype)
            return set_err(GAAST_ERR_INVALID_ARGUMENT, "gather destination: grade set / dimension / dtype differ");
        if (gathered->batch < total) return set_err(GAAST_ERR_INVALID_ARGUMENT, "gather destination holds fewer rows than the ranks send");
        if (gathered->row_stride != gathered->layout.row_len && gathered->batch > 1)
            return set_err(GAAST_ERR_INVALID_ARGUMENT, "gather needs contiguous rows (row_stride == row_len)");
    }
    return GAAST_OK;
}

int chunk_event(int c, hipEvent_t* ev) {
    while (int(g_events.size()) <= c) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        g_events.push_back(e);
    }
    *ev = g_events[size_t(c)];
    return GAAST_OK;
}

// after the last transfer: later work on the library stream (and gaast_hip_synchronize) sees the gathered rows
int join_comm_stream() {
    if (!g_comm_done) HIP_TRY(hipEventCreateWithFlags(&g_comm_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(g_comm_done, g_comm.stream));
    HIP_TRY(hipStreamWaitEvent(g_stream, g_comm_done, 0));
    return GAAST_OK;
}

}  // namespace

extern "C" {

int gaast_hip_eval(gaast_hip_program_t prog, const gaast_hip_mv_t* inputs, int n_inputs, int64_t batch,
                   gaast_hip_mv_t out) {
    if (int st = ensure_init()) return st;
    std::vector<Bound> in_bound;
    if (int st = bind_eval(prog, inputs, n_inputs, batch, out, in_bound)) return st;
    return eval_range(prog, in_bound, out, 0, batch);
}

int gaast_hip_comm_set_library(const char* path) {
    std::string err;
    if (comm_set_library(path, &err)) return rccl_err(err);
    return GAAST_OK;
}

int gaast_hip_comm_unique_id(void* id_out) {
    if (!id_out) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    std::string err;
    if (comm_unique_id(id_out, &err)) return rccl_err(err);
    return GAAST_OK;
}

int gaast_hip_comm_init(const void* id, int rank, int world) {
    if (!id || world < 1 || rank < 0 || rank >= world) return set_err(GAAST_ERR_INVALID_ARGUMENT, "bad communicator argument");
    if (int st = ensure_init()) return st;
    std::string err;
    if (comm_init(g_comm, id, rank, world, &err)) return rccl_err(err);
    return GAAST_OK;
}

int gaast_hip_comm_destroy(void) {
    if (int st = ensure_init()) return st;
    std::string err;
    if (comm_destroy(g_comm, &err)) return rccl_err(err);
    return GAAST_OK;
}

int gaast_hip_comm_info(int* rank, int* world) {
    if (!g_comm.active()) return rccl_err("no communicator: call gaast_hip_comm_init first");
    if (rank) *rank = g_comm.rank;
    if (world) *world = g_comm.world;
    return GAAST_OK;
}

int gaast_hip_comm_count_ranks(int* n_ranks) {
    if (!n_ranks) return set_err(GAAST_ERR_INVALID_ARGUMENT, "null argument");
    if (int st = ensure_init()) return st;
    if (!g_comm.active()) return rccl_err("no communicator: call gaast_hip_comm_init first");
    int64_t* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), sizeof(int64_t)));
    const int64_t one = 1;
    int64_t got = 0;
    std::string err;
    hipError_t e = hipMemcpy(d, &one, sizeof(one), hipMemcpyHostToDevice);
    int failed = 0;
    if (e == hipSuccess) failed = comm_allreduce_sum_i64(g_comm, d, 1, &err);
    if (e == hipSuccess && !failed) e = hipStreamSynchronize(g_comm.stream);
    if (e == hipSuccess && !failed) e = hipMemcpy(&got, d, sizeof(got), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (failed) return rccl_err(err);
    if (e != hipSuccess) return set_err(GAAST_ERR_HIP, std::string("comm_count_ranks: ") + hipGetErrorString(e));
    *n_ranks = int(got);
    return GAAST_OK;
}

int gaast_hip_gather_rows(gaast_hip_mv_t local, gaast_hip_mv_t gathered, const int64_t* counts, int root) {
    if (int st = ensure_init()) return st;
    if (int st = check_gather_args(local, gathered, counts, root)) return st;
    hipEvent_t ev;
    if (int st = chunk_event(0, &ev)) return st;
    HIP_TRY(hipEventRecord(ev, g_stream));               // the rows are produced on the library stream
    HIP_TRY(hipStreamWaitEvent(g_comm.stream, ev, 0));
    if (int st = gather_chunk(local, gathered, counts, root, 1, 0)) return st;
    return join_comm_stream();
}

int gaast_hip_eval_gather(gaast_hip_program_t prog, const gaast_hip_mv_t* inputs, int n_inputs, gaast_hip_mv_t out,
                          gaast_hip_mv_t gathered, const int64_t* counts, int root, int n_chunks) {
    if (int st = ensure_init()) return st;
    if (n_chunks < 1 || n_chunks > 1024) return set_err(GAAST_ERR_INVALID_ARGUMENT, "n_chunks out of range");
    if (int st = check_gather_args(out, gathered, counts, root)) return st;
    const int64_t batch = counts[g_comm.rank];
    if (out->batch != batch) return set_err(GAAST_ERR_INVALID_ARGUMENT, "out must hold counts[rank] items");
    std::vector<Bound> in_bound;
    if (int st = bind_eval(prog, inputs, n_inputs, batch, out, in_bound)) return st;
    // chunk c is computed on the library stream; its rows leave on the communicator's stream while chunk c + 1 is
    // being computed.  Every rank walks all n_chunks steps (a rank with fewer items has empty chunks) so that
    // sends and receives pair up -- also after a local failure: the remaining transfers are still posted (of whatever
    // the rows hold) so that no peer is left waiting in a receive.  The failure is then made COLLECTIVE: every rank
    // all-reduces an error flag and returns non-zero if any rank failed (the root must not hand out stale rows as GAAST_OK).
    int first_error = GAAST_OK;
    std::string first_msg;
    auto note = [&](int st) {
        if (st != GAAST_OK && first_error == GAAST_OK) {
            first_error = st;
            first_msg = g_err;
        }
        return st;
    };
    for (int c = 0; c < n_chunks; ++c) {
        int64_t lo, hi;
        chunk_span(batch, n_chunks, c, &lo, &hi);
        if (first_error == GAAST_OK) note(eval_range(prog, in_bound, out, lo, hi - lo));
        hipEvent_t ev;
        if (note(chunk_event(c, &ev)) == GAAST_OK) {
            if (hipEventRecord(ev, g_stream) != hipSuccess || hipStreamWaitEvent(g_comm.stream, ev, 0) != hipSuccess)
                note(set_err(GAAST_ERR_HIP, "gaast_hip_eval_gather: chunk event"));
        }
        note(gather_chunk(out, gathered, counts, root, n_chunks, c));
    }
    note(join_comm_stream());
    // the collective error flag (sum over the ranks of "I failed"), on the communicator's stream behind the transfers
    int64_t failed_ranks = first_error != GAAST_OK ? 1 : 0;
    {
        std::string err;
        hipError_t e = g_comm_flag ? hipSuccess : hipMalloc(reinterpret_cast<void**>(&g_comm_flag), sizeof(int64_t));
        if (e == hipSuccess) e = hipMemcpy(g_comm_flag, &failed_ranks, sizeof(failed_ranks), hipMemcpyHostToDevice);
        int rc = 0;
        if (e == hipSuccess) rc = comm_allreduce_sum_i64(g_comm, g_comm_flag, 1, &err);
        if (e == hipSuccess && !rc) e = hipStreamSynchronize(g_comm.stream);
        if (e == hipSuccess && !rc) e = hipMemcpy(&failed_ranks, g_comm_flag, sizeof(failed_ranks), hipMemcpyDeviceToHost);
        if (rc) note(rccl_err(err));
        else if (e != hipSuccess) note(set_err(GAAST_ERR_HIP, std::string("gaast_hip_eval_gather: error flag: ") + hipGetErrorString(e)));
    }
    if (first_error != GAAST_OK) return set_err(first_error, first_msg);
    if (failed_ranks > 0)
        return rccl_err("gaast_hip_eval_gather: another rank failed (" + std::to_string(failed_ranks) + " of " + std::to_string(g_comm.world) +
                        "): the gathered rows are not valid");
    return GAAST_OK;
}

}  // extern "C"
