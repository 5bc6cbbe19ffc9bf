// pipeline.hip -- host pipeline + C-ABI of the MI355X SpGEMM backend.
// Role of the reference's MultiplyspECKImplementation (source/GPU/Multiply.cu:51-1122),
// spECKConfig (include/spECKConfig.h) and dCSR helpers (source/dCSR.cpp), re-designed:
//   * one grow-only scratch arena per config (the reference cudaMallocs/frees every
//     scratch buffer inside each call, Multiply.cu:202-225,1056-1070)
//   * the launch sequence is STATIC: every kernel takes its row list and counts from a
//     device-side stats block and its grid depends only on rows(A), so a call needs ONE read-back
//     (nnz(C), to allocate C) instead of the reference's 5-8 -- and NONE in the middle of the call when matOut already
//     holds buffers of the size the previous complete call produced (the through call, option eager_through: the scan
//     checks on the device what the host would have);
//   * a repeated call with the same buffers (the benchmark loop, Executor.cpp:59-72) may REUSE the placement of the
//     previous identical call (option "reuse"; the sequence is enqueued launch by launch -- no executable graph
//     since round 5) -- verified on the device, never trusted; the complete call is what every measurement
//     reports first (bench.py);
//   * kernel classes run concurrently on separate streams between explicit fork/join events.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/speck_c_api.h"
#include "chain3.hpp"
#include "host_common.hpp"
#include "launch.hpp"
#include "row_groups.hpp"
#include "masked.hpp"
#include "select.hpp"
#include "add.hpp"
#include "scale.hpp"
#include "sort_rows.hpp"
#include "tile_scratch.hpp"
#include "coo.hpp"
#include "extract.hpp"
#include "topk.hpp"
#include "sample.hpp"
#include "bmat.hpp"

using namespace speck;

// the launches enqueued since the last check went out (launch.hpp, SPECK_LAUNCH: a failed launch is latched where it
// happens -- the runtime's own "last error" is overwritten by the next successful call)
#define LAUNCHES_OK()                                                                                       \
    do {                                                                                                    \
        if (speck::take_launch_error()) return SPECK_ERR_HIP;                                               \
        HIP_TRY(hipGetLastError());                                                                         \
    } while (0)

namespace speck {
static thread_local int t_launch_error = 0;
void note_launch_status(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    std::fprintf(stderr, "speck_amd: launch of %s failed: %s\n", what, hipGetErrorString(e));
    if (!t_launch_error) t_launch_error = (int)e;
}
int take_launch_error()
{
    const int e = t_launch_error;
    t_launch_error = 0;
    return e;
}
}  // namespace speck

// Everything a reuse sequence is specialised to.
struct CallKey {
    const void* ptr[10] = {};
    u64 num[8] = {};
    bool operator==(const CallKey& o) const
    {
        return std::memcmp(ptr, o.ptr, sizeof(ptr)) == 0 && std::memcmp(num, o.num, sizeof(num)) == 0;
    }
};

// What a complete call leaves behind for a repeated identical call (same buffers, same sizes) to place rows by: the row
// offsets of C -- the config's OWN copy (C.row_offsets is the caller's to overwrite).  The config keeps two: `pred`,
// rewritten by every complete call, and `gpred`, the copy a reuse sequence owns -- a complete call on OTHER buffers in
// between must not change what that sequence compares against (and writes by).
struct Prediction {
    u32* off = nullptr;  // [rows + 1]
    size_t words = 0;
    u32 rows = 0;
};

// What a replayed launch sequence is specialised to: the classes that were non-empty when the same inputs were last
// multiplied eagerly, and what the previous identical call lets it skip.
struct ReplayPlan {
    u32 num_mask, launch_mask;
    u32 num_counts[kMaxClasses];
    bool direct, fused;
    bool skip_scan;  // every kernel that produces a row's nnz compares it with the previous call's (RowWork::verify_counts):
                     //   no scan kernel -- the numeric launches read the records, lists and class table that call's scan left
    bool safe_numeric;  // the numeric launches run in their VERIFYING forms (bounded probing, stores clamped to the row's
                        //   room, counts compared: numeric.hip) -- a reuse sequence walks B before the verdict of the input
                        //   check is read, and the plain forms trust what only a validated B guarantees (every id inside
                        //   the record's column range, the symbolic count = what the table will hold).  Possible when the
                        //   light launch carries no register-class rows of its own; else the check runs FIRST.
    bool num_verify;  // ... and no symbolic pass for the rows of the hash / dense classes: the numeric light launch verifies
                      //   their nnz itself (RowWork::verify_numeric) -- the symbolic phase is the register-class rows alone
    bool overlap;  // the analysis only VERIFIES what the previous identical call left in the arena, on a stream of its
                   //   own beside the symbolic / scan / numeric launches (which read that: DESIGN.md 4.3)
    // ... and everything else of "the last complete call" the launches are sized from: the sequence is enqueued anew at
    // every call and must not pick up what a multiply of ANOTHER problem left in the config since
    u32 sym_mask;
    u32 sym_counts[kMaxClasses];
    u64 g_products, nf_cap_entries;
    u32 nf_wcols;
};

// What the last COMPLETE call on a config left for the next call to be sized from and for a reuse sequence to be planned
// from.  Written by Call::remember_call (a hash one-walk or through call that held refreshes the figures it was chosen by).
struct LastCall {
    bool valid = false;          // such a call has completed ...
    u64 rows_a = 0, rows_b = 0;  // ... on inputs of these shapes
    u32 sym_counts[kMaxClasses] = {}, num_counts[kMaxClasses] = {};  // rows per class
    u32 sym_mask = 0, num_mask = 0;                                  // ... and the classes with rows
    u32 max_row_nnz = 0, max_row_ops = 0;  // its longest row of C, its longest row in products
    u64 g_products = 0;          // what the spill pools were sized for
    u64 nf_entries = 0;          // scratch-pool entries its analysis counted
    bool was_walk = false;       // it was a one-walk call (its nf_entries count the register-class slots too)
    DeviceStats eager_stats{};   // its final statistics block (what `pred` goes with)
    // a complete call of these shapes has run on the config
    bool ran_on(const speck_dcsr* A, const speck_dcsr* B) const { return valid && rows_a == A->rows && rows_b == B->rows; }
};

struct speck_config {
    int device = 0;
    int sm = 0;                 // compute units
    int max_static_lds = 0;
    int max_dynamic_lds = 0;
    std::vector<hipStream_t> streams;  // 6, as in the reference (spECKConfig.h:23-26)
    hipEvent_t completeStart = nullptr, completeEnd = nullptr, individualStart = nullptr,
               individualEnd = nullptr;
    hipStream_t user_stream = nullptr;
    bool use_user_stream = false;

    // scratch arena (device), grow-only
    void* arena = nullptr;
    size_t arena_bytes = 0;
    DeviceStats* d_stats = nullptr;
    DeviceStats* h_stats = nullptr;  // pinned, mapped
    DeviceStats* h_stats_dev = nullptr;  // device address of h_stats
    u32* d_ticket = nullptr;             // completion ticket of a launch sequence: device counter,
    u32* h_ticket = nullptr;             //   pinned host copy (the host spins on it),
    u32* h_ticket_dev = nullptr;         //   its device address
    u32 ticket_expected = 0;
    bool spin_wait = true;
    void* chain_buf = nullptr;           // look-back chain of the analysis / scan kernels (chain.hpp)
    u64 chain_launches = 0;              // ... launches that used it: the tag of the next one (next_chain)
    u32 chain_fault = ~0u;               // test hook (option chain_fault): that workgroup of the NEXT chained launch stays silent
    u64* d_bytes = nullptr;              // [2][kMaxClasses] algorithmic bytes per class (option collect_bytes only)
    ClassifyParams cp{};
    int profile_kernels = 0;  // 1: HIP events around every launch; 2: around the phases only (no event between
                              //    the class launches of a phase)
    std::vector<hipEvent_t> kev;   // kernel event pool (timing)
    std::vector<hipStream_t> aux;  // one stream per kernel class: classes run concurrently
    std::vector<hipEvent_t> aux_done;
    hipEvent_t fork = nullptr;
    hipEvent_t vgate = nullptr;  // behind the analysis launch: the input check of a LARGE B starts there (begin_validate)
    u64 validate_after_nnz = 1ull << 25;  // nnz(B) from which on the check waits for the analysis (option)
    bool eager_speculate = true;  // option eager_speculate: a complete call that follows another one on this config sizes
                                  //   its symbolic phase (grids, launched classes, scratch pool, numeric-first window) from
                                  //   THAT call and runs analysis .. scan as one batch -- one read-back instead of two; the
                                  //   device checks every assumption (capacity_miss: the two-read-back sequence re-runs)
    // option eager_through: ... and when matOut already holds buffers of the size that call produced, the numeric launches are
    // queued right behind the scan -- no read-back in the middle of the call.  The scan checks on the device what the host
    // would have (nnz(C) = what the buffers hold, the classes with rows, the spill pool, the verdict of the input check: its
    // stream is joined in front of the scan); on a miss nothing of C is written and the call re-runs with its read-back.
    bool eager_through = true;
    hipEvent_t vdone = nullptr;         // the input check's stream, joined in front of that scan
    int through_hits = 0, through_misses = 0;
    int eager_spec_hits = 0, eager_spec_misses = 0;
    bool validate_inputs = true;  // complete call: B's rows strictly ascending and in range
    bool concurrent_classes = true;
    u32 max_side_streams = 12;
    float fork_min_us = 60.f;  // estimated duration from which a class launch gets its own stream
    u32 xcd_aware = 10;       // class lists walked in per-XCD contiguous slices: bit 0 sub-wave hash classes,
                              //   bit 1 dense-window / bitmap classes, bit 2 workgroup hash classes, bit 3 the
                              //   register classes (measured: +3.5 % on the cant stand-in for bit 1, -9 % time of
                              //   the small-row launch on the mac_econ stand-in for bit 3 -- that launch is bound by
                              //   its gathers of B rows since it sorts in registers; bits 0 and 2 lose to load
                              //   imbalance)
    LastCall prev;  // what the last complete call left (above)

    // the reuse sequence of the last repeated call (option "reuse")
    bool reuse = true;
    bool plan_valid = false;
    CallKey plan_key;
    CallKey last_key;                         // what the last complete call ran on
    bool last_key_valid = false;
    int replays = 0, plans_made = 0, replay_misses = 0;
    void* gpool = nullptr;    // global-memory buffers of the NUM_G spill path, carved into `spill`
    size_t gpool_bytes = 0;
    void* nfpool = nullptr;   // scratch slots of the numeric-first rows: col_ids | values (grow-only)
    size_t nfpool_bytes = 0;
    u64 nf_cap_entries = 0;
    size_t nf_pool_max_bytes = 0;  // 0: half of the free device memory at allocation time
    int pool_fallbacks = 0;        // times a scratch-pool class was switched off because the pool did not fit
    Prediction pred, gpred;
    bool pred_valid = false;         // pred.off holds the offsets of the last complete call
    bool nf_direct = true;           // option nf_direct: a reuse sequence places its numeric-first rows directly
    bool esc_fused = true;           // option esc_fused: such a sequence finishes the rows of the register classes in
                                     //   its symbolic phase
    ReplayPlan plan{};
    bool skip_scan = true;           // option skip_scan: a reuse sequence that follows a replay of itself has no scan kernel
    int num_verify = 1;              // option num_verify (0: never, 1: when it pays, 2: whenever possible): ... and no symbolic pass for its hash / dense rows (ReplayPlan::num_verify)
    // The inputs the analysis depends on as the last WRITING analysis saw them (stages.hip, launch_snapshot_inputs): A's
    // column ids | B's row offsets | first and last column id of every row of B.  The verifier of a reuse sequence
    // compares the inputs with this copy instead of recomputing the analysis (option verify_inputs); grow-only, and like
    // the arena it belongs to whoever ran a writing analysis last (snap_for_arena travels with arena_key).
    u32* snap = nullptr;
    size_t snap_words = 0, snap_a_words = 0;
    bool verify_inputs = true;
    bool snap_pending = false;       // the verifier of the call in flight recomputes the analysis AND takes the copy
    bool snap_for_arena = false;     // the copy holds the inputs the arena's metadata was derived from (and verified against)
    bool arena_from_replay = false;  // the arena (numeric records, lists, class table, statistics) was last written by a completed
                                     //   REPLAY of arena_key's problem: the layout a sequence without a scan reads
    bool overlap_analysis = true;    // option overlap_analysis: a reuse sequence runs its analysis as a verifier beside it
    hipStream_t vstream = nullptr;   // the verifier's stream
    u32* h_verify = nullptr;         // its verdict (word 0) and its completion ticket (word 16): pinned, mapped
    u32* h_verify_dev = nullptr;
    u32* d_vticket = nullptr;
    u32 vticket_expected = 0;
    bool verifier_in_flight = false; // a verifier / input check runs on vstream: drained on every way out of the call
    bool validate_in_flight = false; // the input check of a complete call is running on vstream (begin_validate)
    CallKey arena_key;              // what the per-row / per-entry metadata in the arena (b_sl, row arrays, records, lists,
    bool arena_key_valid = false;    //   class table) was last written for -- by a multiply that COMPLETED
    u32 nf_wcols = kNumD1Cols;  // LDS window of the numeric-first kernel: the widest such row of the last analysis
    SpillBuffers spill{};
    // debug option guard_bytes (guards.hpp): the zones between the regions carved from the arena / the spill pool, and what
    // layout the arena's were last filled for
    std::vector<GuardZone> arena_zones, gpool_zones, nfpool_zones;
    SortScratch sort;  // temporaries and class limits of speck_sort_rows_* (sort_rows.hip)
    MaskedScratch masked;  // ... and of speck_multiply_masked_* (masked.hip)
    SelectScratch select;  // ... and of speck_select_* (select.hip)
    AddScratch add;  // ... and of speck_add_* (add.hip)
    TileScratch reduce;  // ... and of speck_reduce_* (reduce.hip)
    ScaleScratch scale;  // ... and of speck_scale_* (scale.hip)
    TileScratch spmv;  // ... and of speck_spmv_* (spmv.hip)
    TileScratch spmm;  // ... and of speck_spmm_* (spmm.hip): its own, a spmv after a wide spmm keeps its small buffers
    ScaleScratch sddmm;  // ... and of speck_sddmm_* (sddmm.hip): scale's pair of buffers, its own
    TileScratch softmax;  // ... and of speck_softmax_* (softmax.hip): two sets of tile records, the m and s of the split rows
    TileScratch spmm_t;  // ... and of speck_spmm_t_* (spmm_t.hip): the records of the plan's tiles, the column sums
    TileScratch spmv_sr;  // ... and of speck_spmv_sr_* (semiring.hip)
    TileScratch spmm_sr;  // ... and of speck_spmm_sr_* (semiring.hip): its own, as spmm's is not spmv's
    CooScratch coo;  // ... and of speck_from_coo_* / speck_to_coo (coo.hip): the status block, the keys and buffers of the sort
    ExtractScratch extract;  // ... and of speck_extract_* (extract.hip): the rows' lengths and offsets, the keep bytes
    TopKScratch topk;  // ... and of speck_topk_* (topk.hip): the row lists, the kept entries per row, the new row offsets
    SampleScratch sample;  // ... and of speck_sample_* (sample.hip): the row lists, the rows' sources, lengths and offsets
    BmatScratch bmat;  // ... and of speck_bmat_* (bmat.hip): the tables of blocks and groups, the piece lengths and their scan
    const void* zones_arena = nullptr;
    u64 zones_m = 0, zones_nnz = 0, zones_gap = 0;
    bool gpool_zones_filled = false;
    speck_stats last{};
    // the ONE-WALK complete call (walk.hip; option one_walk): analysis -> symbolic launches of the rows no register class
    // takes -> walk kernel (scan + the register-class rows finished in place) -> the other numeric launches.  Needs C
    // allocated (the caller's matOut of the previous call) and the class counts of the previous complete call for grids.
    int one_walk = 0;                // option: 0 never (default: measured and lost on every stand-in but cant),
                                     //   1 when the previous call says the walk kernel takes a good share of the rows, 2 whenever possible
    int walks = 0, walk_misses = 0;
    // ... and of the HASH classes (numeric.hip, walk_hash_kernel; option one_walk_hash): inputs whose rows all fit the 256-entry
    // sub-wave table (the previous complete call says so) -- analysis -> walk_hash_kernel -> done
    int one_walk_hash = 0;           // (0: off -- measured and lost at full size; 1: when the figures fit; 2: + whatever the row mix)
    u32 walk_hash_debug = 0;
    void* chain3_buf = nullptr;      // three-level chain of that kernel (chain3.hpp): grow-only
    size_t chain3_cap_words = 0;
    u64 chain3_launches = 0;
};

namespace {

// polite busy-wait step of the host thread that waits for the completion ticket
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    asm volatile("" ::: "memory");
#endif
}
constexpr std::chrono::microseconds kSpinBudget{2000};

hipStream_t main_stream(speck_config* c) { return c->use_user_stream ? c->user_stream : c->streams[0]; }

void drop_plan(speck_config* c) { c->plan_valid = false; }

int ensure_arena(speck_config* c, size_t bytes)
{
    if (bytes <= c->arena_bytes) return SPECK_OK;
    drop_plan(c);
    c->last_key_valid = false;
    c->arena_key_valid = false;
    if (c->arena) HIP_TRY(guarded_free(c->arena));
    c->arena = nullptr;
    c->arena_bytes = 0;
    size_t want = bytes + bytes / 4 + (1 << 20);
    HIP_TRY(guarded_malloc(&c->arena, want));
    c->arena_bytes = want;
    return SPECK_OK;
}

// room for the input snapshot of a problem (no room: the verifier recomputes the analysis instead)
void ensure_snap(speck_config* c, u64 nnz_a, u64 b_rows)
{
    const size_t a_words = (size_t(nnz_a) + 63) & ~size_t(63), need = a_words + 3 * size_t(b_rows) + 1;
    if (need > c->snap_words) {
        if (c->snap) (void)guarded_free(c->snap);
        c->snap = nullptr;
        c->snap_words = 0;
        c->snap_for_arena = false;
        const size_t want = need + need / 8;
        if (guarded_malloc(reinterpret_cast<void**>(&c->snap), want * sizeof(u32)) != hipSuccess) {
            (void)hipGetLastError();
            c->snap = nullptr;
            return;
        }
        c->snap_words = want;
    }
    if (c->snap_a_words != a_words) c->snap_for_arena = false;  // (another layout: whatever it holds is not this problem's)
    c->snap_a_words = a_words;
}

struct Carver {
    unsigned char* p;
    size_t used = 0;
    size_t gap;                        // debug option guard_bytes: a canary zone behind every region (guards.hpp)
    std::vector<GuardZone>* zones;     // ... listed here
    explicit Carver(void* base, size_t gap_ = 0, std::vector<GuardZone>* zones_ = nullptr)
        : p(static_cast<unsigned char*>(base)), gap(gap_), zones(zones_) {}
    template <typename U>
    U* take(size_t n)
    {
        size_t bytes = (n * sizeof(U) + 255) & ~size_t(255);
        U* r = reinterpret_cast<U*>(p + used);
        // (the zone starts right behind the last entry of the region, inside its alignment padding)
        if (gap && zones && p) zones->push_back(GuardZone{p + used + n * sizeof(U), bytes - n * sizeof(U) + gap});
        used += bytes + gap;
        return r;
    }
    static size_t need(size_t n, size_t elem) { return ((n * elem + 255) & ~size_t(255)) + guard_bytes(); }
};

struct Scratch {
    u32 *row_ops, *row_max_ops, *row_col_min, *row_col_max;
    RowRec* sym_recs;  // one 32-byte record per row, in the list of its symbolic class (launch.hpp, class_rec_at)
    RowRec* num_recs;  // ... of its numeric class: kept apart, so that the symbolic lists of a call survive its scan (a reuse
                       //   sequence whose analysis only verifies reads those of the previous identical call)
    u8* cls_sym;     // symbolic class of every row
    u32* a_ro_copy;  // A's row offsets as the analysis saw them
    uint2* b_sl;  // per A entry: (start, length) of the referenced B row (written by the analysis)
    uint2* w_sl;  // per A entry: its B entries inside the current column window (multi-window rows)
    u64* nf_off;           // per row: scratch slot of a numeric-first row
    u32* counts;           // per row (+1): nnz of the C row, written by the symbolic kernels
    u32* offsets;          // per row (+1): C.row_offsets of a call until C is known to be allocated
};

size_t scratch_bytes(u32 m, u64 nnz_a)
{
    size_t b = 2 * Carver::need(nnz_a, 8);
    b += 4 * Carver::need(m, 4);
    b += 3 * Carver::need(size_t(m) + 1, 4);
    b += Carver::need(m, 8);
    b += Carver::need(m, 1);
    b += 2 * Carver::need(class_list_records(m), sizeof(RowRec));
    return b + 4096;
}

Scratch carve(speck_config* c, u32 m, u64 nnz_a, std::vector<GuardZone>* zones = nullptr)
{
    Carver cv(c->arena, guard_bytes(), zones);
    Scratch s;
    s.b_sl = cv.take<uint2>(nnz_a);
    s.w_sl = cv.take<uint2>(nnz_a);
    s.nf_off = cv.take<u64>(m);
    s.cls_sym = cv.take<u8>(m);
    s.a_ro_copy = cv.take<u32>(size_t(m) + 1);
    s.row_ops = cv.take<u32>(m);
    s.row_max_ops = cv.take<u32>(m);
    s.row_col_min = cv.take<u32>(m);
    s.row_col_max = cv.take<u32>(m);
    s.counts = cv.take<u32>(size_t(m) + 1);
    s.offsets = cv.take<u32>(size_t(m) + 1);
    s.sym_recs = cv.take<RowRec>(class_list_records(m));
    s.num_recs = cv.take<RowRec>(class_list_records(m));
    return s;
}

// The chain of the next analysis / scan / walk launch on `s`: a tag of its own (chain.hpp).  Two buffers, used in turn: two
// chained launches that follow each other never share descriptors, whatever overlaps them.  A buffer
// is cleared -- on the stream, in front of the launch -- before a tag comes round again.
int next_chain(speck_config* c, hipStream_t s, Chain* out)
{
    Chain ch;
    const u64 turn = c->chain_launches >> 1;
    ch.agg = reinterpret_cast<u64*>(static_cast<unsigned char*>(c->chain_buf) + (c->chain_launches & 1u) * kChainBytes);
    ch.sup = ch.agg + kChainAggWords;
    ch.error = reinterpret_cast<u32*>(ch.sup + kChainSupWords);
    if (turn % kChainTags == 0 && turn != 0) HIP_TRY(hipMemsetAsync(ch.agg, 0, (kChainAggWords + kChainSupWords) * 8, s));
    ch.tag = (u32)(turn % kChainTags) + 1u;
    ch.fault = c->chain_fault;  // (one launch only)
    c->chain_fault = ~0u;
    ++c->chain_launches;
    *out = ch;
    return SPECK_OK;
}
// ... and the three-level chain of the hash one-walk kernel (chain3.hpp) for `groups` workgroups
int next_chain3(speck_config* c, hipStream_t s, u64 groups, Chain3* out)
{
    const size_t words = chain3_words(groups);
    if (words > c->chain3_cap_words) {
        if (c->chain3_buf) (void)guarded_free(c->chain3_buf);
        c->chain3_buf = nullptr;
        c->chain3_cap_words = 0;
        const size_t want = words + words / 8;
        if (guarded_malloc(&c->chain3_buf, want * 8 + 256) != hipSuccess) {
            (void)hipGetLastError();
            return SPECK_ERR_OOM;
        }
        HIP_TRY(hipMemsetAsync(c->chain3_buf, 0, want * 8 + 256, s));
        c->chain3_cap_words = want;
        c->chain3_launches = 0;
    }
    Chain3 ch;
    u64* at = static_cast<u64*>(c->chain3_buf);
    for (u32 k = 0; k < kChain3Levels; ++k) {
        ch.l[k] = at;
        at += chain3_level_words(groups, k);
    }
    ch.error = reinterpret_cast<u32*>(static_cast<u64*>(c->chain3_buf) + c->chain3_cap_words);
    // (the layout depends on `groups`: a word of another launch can only carry ANOTHER tag -- tags are used once per wrap)
    if (c->chain3_launches % kChainTags == 0 && c->chain3_launches != 0)
        HIP_TRY(hipMemsetAsync(c->chain3_buf, 0, c->chain3_cap_words * 8, s));
    ch.tag = (u32)(c->chain3_launches % kChainTags) + 1u;
    ch.fault = c->chain_fault;
    c->chain_fault = ~0u;
    ++c->chain3_launches;
    *out = ch;
    return SPECK_OK;
}
// a wait of a chain timed out (DeviceStats::chain_error): the call returns SPECK_ERR_HIP; the flags are cleared so that
// the NEXT call on the config starts clean
int chain_failed(speck_config* c, hipStream_t s)
{
    for (int k = 0; k < 2; ++k)
        (void)hipMemsetAsync(static_cast<unsigned char*>(c->chain_buf) + k * kChainBytes + (kChainAggWords + kChainSupWords) * 8, 0, 4, s);
    if (c->chain3_buf) (void)hipMemsetAsync(static_cast<u64*>(c->chain3_buf) + c->chain3_cap_words, 0, 4, s);
    (void)hipStreamSynchronize(s);
    return SPECK_ERR_HIP;
}

// (re)allocate a Prediction for `m` rows; false if the device has no room (the reuse sequence then places nothing)
bool ensure_pred(Prediction& p, u32 m)
{
    const size_t need = size_t(m) + 1;
    if (need > p.words) {
        if (p.off) (void)guarded_free(p.off);
        p = Prediction{};
        if (guarded_malloc(reinterpret_cast<void**>(&p.off), need * 4) != hipSuccess) {
            (void)hipGetLastError();
            p.off = nullptr;
            return false;
        }
        p.words = need;
    }
    p.rows = m;
    return true;
}

// scratch pool of the numeric-first rows: `entries` column ids followed by `entries` values
int ensure_nfpool(speck_config* c, u64 entries, size_t vsize)
{
    const size_t need = Carver::need(entries, 4) + Carver::need(entries, vsize) + 512;
    if (entries <= c->nf_cap_entries && need <= c->nfpool_bytes) return SPECK_OK;
    drop_plan(c);
    c->last_key_valid = false;
    if (c->nfpool) (void)guarded_free(c->nfpool);
    c->nfpool = nullptr;
    c->nfpool_bytes = 0;
    c->nf_cap_entries = 0;
    const u64 cap = entries + entries / 8 + 1024;
    const size_t bytes = Carver::need(cap, 4) + Carver::need(cap, 8) + 512;
    // budget: an explicit cap (option nf_pool_max_mb) or half of what the device has free -- hidden scratch must
    // not be what makes a later allocation of C fail
    size_t free_b = 0, total_b = 0;
    size_t budget = c->nf_pool_max_bytes;
    if (!budget && hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = free_b / 2;
    if (budget && bytes > budget) return SPECK_ERR_OOM;
    if (guarded_malloc(&c->nfpool, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return SPECK_ERR_OOM;
    }
    c->nfpool_bytes = bytes;
    c->nf_cap_entries = cap;
    c->nfpool_zones.clear();
    if (guard_bytes()) {  // between the column ids and the values, behind the values
        unsigned char* b = static_cast<unsigned char*>(c->nfpool);
        c->nfpool_zones.push_back(GuardZone{b + cap * 4, Carver::need(cap, 4) - cap * 4});
        c->nfpool_zones.push_back(GuardZone{b + Carver::need(cap, 4) + cap * 8, bytes - Carver::need(cap, 4) - cap * 8});  // (behind 8-byte values: a float call uses half)
        if (guard_fill(c->nfpool_zones, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return SPECK_ERR_HIP;
    }
    return SPECK_OK;
}

int begin_validate(speck_config* c, const speck_dcsr* B, hipStream_t gate = nullptr);

// The input check of a complete call, started once: behind the launch of the analysis, the head of the call's critical
// path, and beside that latency-bound kernel rather than beside the symbolic launches
struct InputCheck {
    speck_config* c;
    const speck_dcsr* B;
    hipStream_t s;
    bool started = false;
    int start()
    {
        if (!c->validate_inputs || started) return SPECK_OK;
        started = true;
        return begin_validate(c, B, s);
    }
};

// What kind of call is being enqueued.  Whoever enqueues builds one on the stack and hands it to make_work,
// enqueue_front and enqueue_back: it is gone with the call.  Default: a plain complete call, nothing staged.
struct CallForm {
    // a reuse sequence (enqueue_replay maps its ReplayPlan onto these): rows placed where the previous identical call put
    // them | register-class rows finished in the symbolic phase | no analysis IN the sequence, A's offsets are the arena's
    // copy | no scan kernel | the numeric launches in their verifying forms
    bool direct = false, fused = false, overlap = false, skip_scan = false, num_verify = false;
    bool one_walk = false;  // the one-walk complete call (walk.hip)
    u32* c_col = nullptr;   // C's buffers, for the rows placed early (direct, one_walk) ...
    void* c_val = nullptr;
    u64 c_cap = 0;          // ... and the entries they hold (one_walk)
    const u32* off_src = nullptr;  // the staged row offsets ride to C in the numeric light launch (RowWork::off_src)
    u32* off_dst = nullptr;
    u32 off_n = 0;
    const u32* through_gate = nullptr;     // through call: the verdict word of the input check, which the scan looks at
    u32 through_ticket = 0;                // != 0: ... and the ticket the check stores when it is done (its stream is not joined)
    InputCheck* after_analysis = nullptr;  // complete call: started behind the launch of the analysis
    u32 nf_wcols = kNumD1Cols;             // LDS window of the numeric-first kernel: c->nf_wcols, or a plan's
};

RowWork make_work(speck_config* c, const Scratch& sc, const SpillBuffers& spill, u32 m, const CallForm& f,
                  bool symbolic_phase = false)
{
    RowWork w{};
    w.recs = symbolic_phase ? sc.sym_recs : sc.num_recs;
    w.m = m;
    w.st = c->d_stats;
    w.b_sl = sc.b_sl;
    w.spill = spill;
    w.nf_off = sc.nf_off;
    w.nf_col = static_cast<u32*>(c->nfpool);
    w.nf_val = c->nfpool ? static_cast<unsigned char*>(c->nfpool) + Carver::need(c->nf_cap_entries, 4) : nullptr;
    w.nf_cap = c->nfpool ? c->nf_cap_entries : 0;
    w.nf_pred_off = (f.direct || f.skip_scan) ? c->gpred.off : nullptr;
    w.nf_direct_col = f.direct ? f.c_col : nullptr;
    w.nf_direct_val = f.direct ? f.c_val : nullptr;
    w.w_sl = sc.w_sl;
    w.xcd_aware = c->xcd_aware;
    w.off_src = symbolic_phase ? nullptr : f.off_src;
    w.off_dst = symbolic_phase ? nullptr : f.off_dst;
    w.off_n = symbolic_phase ? 0u : f.off_n;
    w.verify_counts = f.skip_scan ? 1u : 0u;
    w.verify_numeric = f.num_verify ? 1u : 0u;
    return w;
}

struct StageTimer {
    speck_config* c;
    bool on;
    hipStream_t s;
    StageTimer(speck_config* cfg, bool enable, hipStream_t st) : c(cfg), on(enable), s(st)
    {
        if (on) start();
    }
    void start() { (void)hipEventRecord(c->individualStart, s); }
    // returns ms since start() and restarts (reference: recordTimerVar/startTimerVar,
    // source/GPU/Multiply.cu:36-49)
    float lap()
    {
        if (!on) return 0.f;
        float ms = 0.f;
        (void)hipEventRecord(c->individualEnd, s);
        (void)hipEventSynchronize(c->individualEnd);
        (void)hipEventElapsedTime(&ms, c->individualStart, c->individualEnd);
        start();
        return ms;
    }
};

// The walks over a row of A (for_each_product, WindowCursors, the analysis' walk_entries, the register classes) count its
// entries in u32 and step by up to 2^11 entries (the eight waves of the analysis, four tiles of 64 each): behind entry 2^32 - 1 such a counter starts
// over at 0.  A row-range view of A whose entries reach the last 2^16 below 2^32 is therefore refused before any kernel
// starts.  Entries that high exist only in an allocation that holds them: the runtime says how far col_ids reaches, and
// row_offsets[0] is read back (4 bytes, the stream waited for) only where it reaches that far -- 16 GiB of column ids.
constexpr u64 kViewTopMargin = 1ull << 16;

int check_view_below_the_top(const speck_dcsr* A, hipStream_t s)
{
    constexpr u64 limit = (1ull << 32) - kViewTopMargin;
    if (!A->rows || !A->nnz || !A->col_ids) return SPECK_OK;
    if (A->nnz > limit) return SPECK_ERR_INVALID;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)A->col_ids) == hipSuccess) {
        const u64 reach = (u64(reinterpret_cast<uintptr_t>(base)) + size - u64(reinterpret_cast<uintptr_t>(A->col_ids))) / 4;
        if (reach <= limit) return SPECK_OK;
    } else {
        (void)hipGetLastError();  // (not an allocation the runtime knows: ask the offsets)
    }
    u32 first = 0;
    HIP_TRY(hipMemcpyAsync(&first, A->row_offsets, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return u64(first) + A->nnz > limit ? SPECK_ERR_INVALID : SPECK_OK;
}

int check_inputs(const speck_dcsr* A, const speck_dcsr* B)
{
    if (!A || !B) return SPECK_ERR_INVALID;
    if (A->cols != B->rows) return SPECK_ERR_INVALID;
    // reference limits, source/GPU/Multiply.cu:57-66 (hash key / block-range packing);
    // kept so that every input the reference accepts is accepted and vice versa
    if (B->cols > (1ull << 27) || A->rows > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->rows && !A->row_offsets) return SPECK_ERR_INVALID;
    if (B->rows && !B->row_offsets) return SPECK_ERR_INVALID;
    return SPECK_OK;
}

hipEvent_t kernel_event(speck_config* c, size_t i)
{
    while (c->kev.size() <= i) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        c->kev.push_back(e);
    }
    return c->kev[i];
}

// The call's value type for code that is a template of it: f(T{}) with T = double / float by the size of a value
template <typename F>
auto with_value_type(u32 vsize, F&& f)
{
    return vsize == 8 ? f(double{}) : f(float{});
}
template <typename T>
CsrView<T> view_of(const speck_dcsr* M)
{
    return {M->row_offsets, M->col_ids, static_cast<const T*>(M->data), (u32)M->rows, (u32)M->cols};
}

struct ClassTiming {
    int cls;
    size_t ev;
};

// Launch the items of `order` (kSymOrder / kNumOrder, launch.hpp) that have rows by `mask`: the heavy classes, each with
// launches of its own, and kLight, the ONE launch of the classes in `light_mask`.  The items are independent (disjoint
// rows), so each may run on its own stream between a fork and a join event on the pipeline stream: the
// latency-bound heavy-row kernels (few workgroups) overlap the throughput-bound small-row ones
// (the reference does the same with its 6 streams, source/GPU/Multiply.cu:494-553, but relies on
// legacy default-stream ordering; here the dependencies are explicit events).
template <int n_order, typename LaunchFn>
int run_classes(speck_config* c, hipStream_t s, const int (&order)[n_order], u32 mask, u32 light_mask,
                const u32* counts, const float* ns_per_row, size_t* ev_idx, std::vector<ClassTiming>* timing,
                int exact_cls, LaunchFn&& launch)
{
    bool forked = false;
    size_t used = 0;
    auto active = [&](int cls) { return cls == kLight ? (mask & light_mask) != 0 : (mask >> cls & 1u) != 0; };
    // Estimated duration of an item from the host-known row counts of the previous identical call
    // (isolated per-row costs, scripts/class_times.py).  An item earns a side stream only when it is
    // long enough to pay for the cross-queue dependency (~10-15 us per branch):
    // the scircuit / mac_econ stand-ins run fastest on ONE stream, the webbase one with four.
    auto est_us = [&](int cls) -> float {
        if (!counts) return 1e9f;  // first call: counts unknown, keep every class apart
        const u32 m = cls == kLight ? (mask & light_mask) : (1u << cls);
        float us = 0.f;
        for (int k = 0; k < kMaxClasses; ++k)
            if (m >> k & 1u) us += counts[k] * ns_per_row[k] * 1e-3f;
        return us;
    };
    int n_big = 0;
    for (int i = 0; i < n_order; ++i)
        if (active(order[i]) && est_us(order[i]) >= c->fork_min_us) ++n_big;
    // The last active item stays on the pipeline stream: a fork costs its branch 10-20 us of
    // cross-queue latency, a join on an already finished branch almost nothing -- so a phase with
    // one kernel pays no event at all, and the merged light launch (usually the longest) starts
    // at once while the heavy-row kernels start late on their side streams and still finish first.
    int last_active = -1;
    for (int i = 0; i < n_order; ++i)
        if (active(order[i])) last_active = i;
    // ... and the last LONG one if there are several (the short ones queue on the pipeline stream too)
    if (n_big >= 2)
        for (int i = 0; i < n_order; ++i)
            if (active(order[i]) && est_us(order[i]) >= c->fork_min_us) last_active = i;
    // at most `max_side_streams` branches: further side items queue behind each other on the last side stream
    const size_t max_side = std::min<size_t>(c->aux.size(), c->max_side_streams);
    size_t touched = 0;  // side streams that carry work
    // The HOST needs ~5 us per launch, and a phase of the webbase stand-in is a dozen of them (the spill chain alone is
    // nine): the items are enqueued LONGEST FIRST -- in the fixed order of rounds 1-4 the two NUM_B8K launches, which end
    // that phase, were enqueued 55 us after the scan's ticket, behind the short kernels of the spill chain.
    int seq[kMaxClasses + 2];
    int n_seq = 0;
    for (int i = 0; i < n_order; ++i)
        if (active(order[i])) seq[n_seq++] = i;
    if (counts)
        std::stable_sort(seq, seq + n_seq, [&](int a, int b) { return est_us(order[a]) > est_us(order[b]); });
    auto on_side = [&](int i) {
        return c->concurrent_classes && max_side > 0 && i != last_active && n_big >= 2 && est_us(order[i]) >= c->fork_min_us;
    };
    // (the fork is recorded in front of EVERYTHING the phase puts on the pipeline stream: a side item must not wait for
    //  the pipeline stream's own item of the phase)
    for (int q = 0; q < n_seq && !forked; ++q)
        if (on_side(seq[q])) {
            HIP_TRY(hipEventRecord(c->fork, s));
            forked = true;
        }
    for (int q = 0; q < n_seq; ++q) {
        const int i = seq[q];
        const int cls = order[i];
        hipStream_t ks = s;
        if (on_side(i)) {
            const size_t slot = std::min(used, max_side - 1);
            ks = c->aux[slot];
            if (slot >= touched) {
                HIP_TRY(hipStreamWaitEvent(ks, c->fork, 0));
                touched = slot + 1;
            }
            ++used;
        }
        const bool timed = c->profile_kernels == 1 && timing;
        // the light launches and the numeric-first one stamp their events themselves, with the kernel's own begin and
        // end (launch.hpp, SPECK_LAUNCH_TIMED); the others are bracketed by two event records
        const bool exact = timed && (cls == kLight || cls == exact_cls);
        hipEvent_t e0 = timed ? kernel_event(c, *ev_idx) : nullptr, e1 = timed ? kernel_event(c, *ev_idx + 1) : nullptr;
        if (timed && !exact) (void)hipEventRecord(e0, ks);
        launch(ks, cls, exact ? e0 : nullptr, exact ? e1 : nullptr);
        if (timed) {
            if (!exact) (void)hipEventRecord(e1, ks);
            timing->push_back({cls, *ev_idx});
            *ev_idx += 2;
        }
    }
    for (size_t k = 0; k < touched; ++k) {
        HIP_TRY(hipEventRecord(c->aux_done[k], c->aux[k]));
        HIP_TRY(hipStreamWaitEvent(s, c->aux_done[k], 0));
    }
    LAUNCHES_OK();
    return SPECK_OK;
}

// isolated cost per row of every class (ns, MI355X, scripts/class_times.py on the four stand-ins), in the order of
// SymClass / NumClass (device_common.hpp)
constexpr float kSymNsPerRow[kMaxClasses] = {0.15f, 0.6f, 3.f, 5.f, 30.f, 1000.f, 8.5f, 1000.f, 12.f, 50000.f, 0.1f, 0.4f,
                                             0.4f, 0.8f, 0.f, 0.f};
constexpr float kNumNsPerRow[kMaxClasses] = {0.1f, 0.3f, 2.f, 4.f, 12.f, 75.f, 12.f, 300.f, 1500.f, 2.5f, 1.5f, 0.2f,
                                             0.6f, 1.2f, 0.f, 0.f};
constexpr u32 kAllSym = (1u << SYM_CLASSES) - 1u;
constexpr u32 kAllNum = (1u << NUM_CLASSES) - 1u;

u32 mask_of(const u32* counts, int n)
{
    u32 m = 0;
    for (int i = 0; i < n; ++i)
        if (counts[i]) m |= 1u << i;
    return m;
}

struct Timing {
    size_t ev = 0, ev_analysis = 0, ev_analysis_end = 0, ev_scan = 0, ev_num = 0;
    std::vector<ClassTiming> sym, num;
};

// What enqueue_front is given beside the form; the defaults are a plain complete call's.
struct FrontArgs {
    u64 exact_nnz = ~0ull;  // nnz(C) the scan insists on
    u32 sym_mask = kAllSym, num_mask = kAllNum;
    bool classify_numeric = true;
    const u32* sym_hint = nullptr;  // rows per symbolic class: grids, fork decisions
    bool hint_exact = true;         // ... and they are THIS call's counts
    DeviceStats* host_mirror = nullptr;
    u64 expect_g = ~0ull, expect_nf = ~0ull;
    u32 expect_g_rows = ~0u;
    u32 parts = 3;                // 1: analysis + binning, 2: symbolic launches + scan
    u32* pred_off_out = nullptr;  // what this call leaves for a repeated one to place rows by
};

// analysis (+ symbolic binning) -> symbolic classes -> scan (+ numeric binning).  Nothing here needs a host
// decision: `sym_mask` only prunes kernels of classes known to be empty (first call: all).
int enqueue_front(speck_config* c, hipStream_t s, const speck_dcsr* A_in, const speck_dcsr* B, const Scratch& sc,
                  u32 vsize, const CallForm& f, const FrontArgs& a, Timing* tm)
{
    const u32 m = (u32)A_in->rows;
    const u32 sym_mask = a.sym_mask;
    const u32* const sym_hint = a.sym_hint;
    // A sequence whose analysis only verifies (CallForm::overlap) reads A's row offsets where the previous identical call
    // left them, like the rest of the structure-derived metadata: whatever the caller does to A.row_offsets while the
    // sequence runs, its kernels see ONE consistent structure, and the verifier says whether it is still A's.
    speck_dcsr a_stored = *A_in;
    if (f.overlap) a_stored.row_offsets = sc.a_ro_copy;
    const speck_dcsr* const A = &a_stored;
    u32* const c_ro = sc.counts;  // the symbolic kernels count into scratch; the scan writes sc.offsets
    ClassifyParams cp = c->cp;
    cp.sym_allowed = sym_mask;
    cp.num_allowed = a.num_mask;
    cp.esc16 = (c->cp.esc16 && B->cols <= (1ull << 26)) ? 1u : 0u;  // (column << 6 | product number) fits 32 bits
    cp.esc_fused = f.fused ? 1u : 0u;
    cp.one_walk = f.one_walk ? 1u : 0u;
    cp.slice_ops = (c->cp.slice_ops && u64(B->cols) <= kSliceMaxCols) ? c->cp.slice_ops : 0u;  // (as enqueue_back launches)
    if (f.one_walk) {  // (the walk kernel takes the register-class rows and moves the numeric-first ones itself)
        cp.sym_allowed |= kSymEscMask;
        cp.num_allowed |= kNumEscMask | (1u << NUM_NFCOPY);
    }
    u64* const bytes = c->cp.want_bytes ? c->d_bytes : nullptr;
    const bool timed = c->profile_kernels && tm;
    if (a.parts & 1u) {
        if (timed) {
            tm->ev_analysis = tm->ev;
            (void)hipEventRecord(kernel_event(c, tm->ev++), s);
        }
        // (overlap: no analysis IN the sequence -- launch_verifier puts it on a stream of its own)
        if (!f.overlap) {
            if (bytes) HIP_TRY(hipMemsetAsync(bytes, 0, 2 * kMaxClasses * sizeof(u64), s));
            Chain chain;
            const int crc = next_chain(c, s, &chain);
            if (crc != SPECK_OK) return crc;
            launch_analysis(s, A->row_offsets, A->col_ids, B->row_offsets, B->col_ids, m, A->nnz, sc.row_ops,
                            sc.row_max_ops, sc.row_col_min, sc.row_col_max, sc.cls_sym, c_ro, sc.sym_recs,
                            c->d_stats, cp, sc.b_sl, chain, sc.nf_off, a.expect_nf, (u32)B->rows, sc.a_ro_copy, nullptr, bytes,
                            B->nnz);
            c->snap_for_arena = false;  // (a writing analysis: the copy of the inputs is not its)
        }
        // (complete call: the input check of B goes onto its stream HERE)
        if (f.after_analysis) {
            const int hrc = f.after_analysis->start();
            if (hrc != SPECK_OK) return hrc;
        }
        if (timed) {
            tm->ev_analysis_end = tm->ev;
            (void)hipEventRecord(kernel_event(c, tm->ev++), s);
        }
        LAUNCHES_OK();
    }
    if (!(a.parts & 2u)) return SPECK_OK;
    const RowWork w = make_work(c, sc, SpillBuffers{}, m, f, true);
    // heaviest classes first: they have the longest tails
    u32 all_m[kMaxClasses];
    for (auto& x : all_m) x = m;  // no host-known counts: size every class for rows(A)
    const u32* hint = sym_hint ? sym_hint : all_m;
    int rc = run_classes(c, s, kSymOrder, sym_mask, kSymLightMask, sym_hint, kSymNsPerRow, tm ? &tm->ev : nullptr,
                         tm ? &tm->sym : nullptr, (int)SYM_NF,
                         [&](hipStream_t ks, int cls, hipEvent_t e0, hipEvent_t e1) {
                             if (cls == kLight) {
                                 launch_symbolic_light(ks, hint, sym_mask & kSymLightMask, A->row_offsets, sc.b_sl, B->col_ids, w,
                                                       c_ro, c->sm, sym_hint != nullptr && a.hint_exact,
                                                       f.fused ? vsize : 0u, A->data, B->data, e0, e1);
                             } else if (cls == SYM_NF) {
                                 // the numeric dense-window kernel, in the symbolic phase (numeric.hip)
                                 with_value_type(vsize, [&](auto t) {
                                     using T = decltype(t);
                                     launch_numeric_first<T>(ks, hint[cls], view_of<T>(A), view_of<T>(B), w, c_ro, c->sm,
                                                             f.nf_wcols, e0, e1);
                                 });
                             } else
                                 launch_symbolic(ks, cls, hint[cls], A->row_offsets, sc.b_sl,
                                                 B->col_ids, w, c_ro, c->sm);
                         });
    if (rc != SPECK_OK) return rc;
    if (f.one_walk) {
        // the walk kernel: scan + numeric binning + the numeric walk of the register-class rows (walk.hip); its events
        // carry the kernel's own begin and end
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) {
            tm->ev_scan = tm->ev;
            e0 = kernel_event(c, tm->ev++);
            e1 = kernel_event(c, tm->ev++);
        }
        Chain chain;
        const int crc = next_chain(c, s, &chain);
        if (crc != SPECK_OK) return crc;
        WalkArgs wa{};
        wa.a_ro = A->row_offsets;
        wa.row_ops = sc.row_ops, wa.row_col_min = sc.row_col_min, wa.row_col_max = sc.row_col_max;
        wa.cls_sym = sc.cls_sym;
        wa.counts = c_ro;
        wa.nf_off = sc.nf_off;
        wa.offsets_out = sc.offsets;
        wa.pred_off_out = a.pred_off_out;
        wa.recs = sc.num_recs;
        wa.st = c->d_stats;
        wa.c_col = f.c_col;
        wa.c_val = f.c_val;
        wa.c_cap = f.c_cap;
        wa.pool_col = w.nf_col;
        wa.pool_val = w.nf_val;
        wa.pool_cap = w.nf_cap;
        wa.m = m;
        wa.vsize = vsize;
        wa.cp = cp;
        wa.expect_g = a.expect_g;
        wa.expect_g_rows = a.expect_g_rows;
        wa.bytes_acc = bytes;
        with_value_type(vsize, [&](auto t) {
            using T = decltype(t);
            const ProductSrc<T> src{sc.b_sl, static_cast<const T*>(A->data), B->col_ids, static_cast<const T*>(B->data), sc.w_sl};
            launch_walk<T>(s, wa, src, chain, e0, e1);
        });
        LAUNCHES_OK();
        return SPECK_OK;
    }
    if (timed) {
        tm->ev_scan = tm->ev;
        (void)hipEventRecord(kernel_event(c, tm->ev++), s);
    }
    if (f.skip_scan) {
        // no scan: every row's nnz was compared with the previous call's where it was produced (store_row_count, the
        // fused register-class bodies, the numeric-first kernel); the numeric launches read what that call's scan left
    } else {
        Chain chain;
        const int crc = next_chain(c, s, &chain);
        if (crc != SPECK_OK) return crc;
        // (through call: the input check finished long ago, or at least before this scan.  A LARGE B: its stream is joined;
        //  else the scan looks for the check's ticket -- a join costs ~6 us of this short call even on a finished branch)
        if (f.through_gate && !f.through_ticket) {
            HIP_TRY(hipEventRecord(c->vdone, c->vstream));
            HIP_TRY(hipStreamWaitEvent(s, c->vdone, 0));
        }
        launch_scan(s, c_ro, sc.offsets, m, A->row_offsets, sc.row_ops, sc.row_col_min, sc.row_col_max,
                    a.classify_numeric ? sc.num_recs : nullptr, c->d_stats, cp, vsize, a.exact_nnz, chain, a.host_mirror,
                    a.expect_g, a.expect_g_rows, f.direct ? c->gpred.off : nullptr, a.pred_off_out,
                    a.host_mirror ? c->d_ticket : nullptr, a.host_mirror ? c->h_ticket_dev : nullptr, bytes,
                    f.through_gate, f.through_ticket);
    }
    if (timed) (void)hipEventRecord(kernel_event(c, tm->ev++), s);
    LAUNCHES_OK();
    return SPECK_OK;
}

template <typename T>
int enqueue_back(speck_config* c, hipStream_t s, const speck_dcsr* A, const speck_dcsr* B,
                 const Scratch& sc, const CallForm& f, u32* c_col, T* c_val, u32 num_mask,
                 const u32* counts /*host-known, or nullptr*/, Timing* tm)
{
    const u32 m = (u32)A->rows;
    CsrView<T> Av = view_of<T>(A);
    const CsrView<T> Bv = view_of<T>(B);
    if (f.overlap) Av.row_offsets = sc.a_ro_copy;  // (as enqueue_front: the structure the sequence was built on)
    RowWork w = make_work(c, sc, c->spill, m, f);
    w.sliced = (c->cp.slice_ops && u64(B->cols) <= kSliceMaxCols) ? 1u : 0u;  // (as enqueue_front classifies)
    // the staged offsets -> C.row_offsets: by extra workgroups of the numeric light launch when there is one, else by a
    // (guarded) copy of its own
    if (w.off_n && !(num_mask & kNumLightMask)) {
        launch_copy_offsets(s, w.off_src, w.off_dst, w.off_n, c->d_stats);
        w.off_n = 0;
    }
    u32 all_m[kMaxClasses];
    for (auto& x : all_m) x = m;
    const u32* hint = counts ? counts : all_m;
    return run_classes(c, s, kNumOrder, num_mask, kNumLightMask, counts, kNumNsPerRow, tm ? &tm->ev : nullptr,
                       tm ? &tm->num : nullptr, -100,
                       [&](hipStream_t ks, int cls, hipEvent_t e0, hipEvent_t e1) {
                           if (cls == kLight)
                               launch_numeric_light<T>(ks, hint, num_mask & kNumLightMask, Av, Bv, w, c_col, c_val, c->sm,
                                                       counts != nullptr, e0, e1);
                           else
                               launch_numeric<T>(ks, cls, hint[cls], Av, Bv, w, c_col, c_val, c->sm);
                       });
}

// Wait for everything enqueued on `s` behind a done_kernel (launch_done): the host spins on the ticket that kernel
// stores into pinned memory (bounded by TIME -- work that is still running after kSpinBudget is long enough for the
// wake-up latency of the blocking call not to matter -- then the blocking synchronisation).
int wait_ticket(speck_config* c, hipStream_t s)
{
    if (c->spin_wait) {
        const u32 want = ++c->ticket_expected;
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        while (!(seen = __atomic_load_n(c->h_ticket, __ATOMIC_ACQUIRE) == want)) {
            for (int i = 0; i < 64; ++i) cpu_relax();
            if (std::chrono::steady_clock::now() - t0 > kSpinBudget) break;
        }
        if (!seen) HIP_TRY(hipStreamSynchronize(s));
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    c->ticket_expected = __atomic_load_n(c->h_ticket, __ATOMIC_ACQUIRE);
    return SPECK_OK;
}

// The statistics block of the call so far, on the host.  With the ticket: done_kernel mirrors the block into pinned
// memory and the host spins (a copy + blocking synchronisation costs 10-20 us of wake-up latency).
int read_stats(speck_config* c, hipStream_t s)
{
    if (c->spin_wait) {
        launch_done(s, c->d_ticket, c->h_ticket_dev, c->d_stats, c->h_stats_dev);
        const int rc = wait_ticket(c, s);
        if (rc != SPECK_OK) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(c->h_stats, c->d_stats, sizeof(DeviceStats), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return c->h_stats->chain_error ? chain_failed(c, s) : SPECK_OK;
}

// ... when the scan of the batch mirrors the block and stores the ticket itself (enqueue_front with a host mirror):
// no done_kernel, the host has the statistics while the scan's other tiles are still writing their rows
int await_scan_stats(speck_config* c, hipStream_t s)
{
    if (!c->spin_wait) return read_stats(c, s);
    const int rc = wait_ticket(c, s);
    if (rc != SPECK_OK) return rc;
    return c->h_stats->chain_error ? chain_failed(c, s) : SPECK_OK;
}

void publish_counts(speck_config* c, hipStream_t s)
{
    c->last.sum_products = c->h_stats->sum_products;
    c->last.max_row_ops = c->h_stats->max_row_ops;
    c->last.nnz_c = c->h_stats->nnz_c;
    c->last.max_row_nnz_c = c->h_stats->max_row_nnz_c;
    for (int i = 0; i < SPECK_NUM_SYM_BINS; ++i) c->last.sym_bin_rows[i] = c->h_stats->sym.count[i];
    for (int i = 0; i < SPECK_NUM_NUM_BINS; ++i) c->last.num_bin_rows[i] = c->h_stats->num.count[i];
    if (c->cp.want_bytes && c->d_bytes) {  // (profiling: the per-class byte model, summed by the analysis / scan kernels)
        u64 b[2 * kMaxClasses] = {};
        if (hipStreamSynchronize(s) == hipSuccess && hipMemcpy(b, c->d_bytes, sizeof(b), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int i = 0; i < SPECK_NUM_SYM_BINS; ++i) c->last.sym_bin_bytes[i] = b[i];
            for (int i = 0; i < SPECK_NUM_NUM_BINS; ++i) c->last.num_bin_bytes[i] = b[kMaxClasses + i];
        }
    }
}

template <typename T>
CallKey make_key(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* C,
                  hipStream_t s)
{
    CallKey k;
    k.ptr[0] = A->row_offsets; k.ptr[1] = A->col_ids; k.ptr[2] = A->data;
    k.ptr[3] = B->row_offsets; k.ptr[4] = B->col_ids; k.ptr[5] = B->data;
    k.ptr[6] = C->row_offsets; k.ptr[7] = C->col_ids; k.ptr[8] = C->data;
    k.ptr[9] = c->arena;
    k.num[0] = A->rows; k.num[1] = A->nnz; k.num[2] = B->rows; k.num[3] = B->cols; k.num[4] = C->nnz;
    k.num[5] = sizeof(T);
    k.num[6] = (u64(c->cp.sym_bitmap_ratio) << 32) | c->cp.num_dense_ratio;
    k.num[7] = (u64(c->cp.num_global_passes) << 32) | (u64(c->cp.sym_w128) << 5) | (u64(c->cp.sym_g8) << 4) | (u64(c->cp.num_g8) << 3) | (u64(c->cp.num_w256) << 2) |
               (u64(c->cp.want_bytes) << 1) |
               (c->concurrent_classes ? 1u : 0u);
    k.num[7] ^= reinterpret_cast<u64>(s);
    k.num[5] |= u64(c->cp.nf_min_ops) << 8;
    k.num[5] |= (u64(c->cp.esc32) << 40) | (u64(c->cp.esc64) << 41) | (u64(c->cp.esc16) << 42);
    k.num[4] |= u64(c->cp.gh_per_window) << 32;  // C->nnz fits 32 bits
    return k;
}

// The config's copy of the row offsets (of the last complete call = this call: same key) becomes the sequence's own.
int snapshot_prediction(speck_config* c, hipStream_t s)
{
    if (!c->pred_valid) return SPECK_OK;
    if (!ensure_pred(c->gpred, c->pred.rows)) return SPECK_ERR_OOM;
    HIP_TRY(hipMemcpyAsync(c->gpred.off, c->pred.off, (size_t(c->pred.rows) + 1) * 4, hipMemcpyDeviceToDevice, s));
    return SPECK_OK;
}

// What a repeated identical call may take from the previous one (DESIGN.md 3, table of pred_stages bits).  FROZEN since
// round 5: the complete call is what is measured; this mode is kept, tested, and not extended.
ReplayPlan plan_replay(const speck_config* c, bool arena_mine, bool arena_replay_ok)
{
    ReplayPlan p;
    p.num_mask = c->prev.num_mask;
    std::memcpy(p.num_counts, c->prev.num_counts, sizeof(p.num_counts));
    p.sym_mask = c->prev.sym_mask;
    std::memcpy(p.sym_counts, c->prev.sym_counts, sizeof(p.sym_counts));
    p.g_products = c->prev.g_products;
    p.nf_cap_entries = c->nf_cap_entries;
    p.nf_wcols = c->nf_wcols;
    // Numeric-first rows: a complete call writes them to scratch slots and copies them after the scan (nothing else
    // knows where a row goes before the scan).  The reuse sequence knows where they WENT: it writes each row
    // straight to the offset the previous identical call gave it, provided its fresh nnz is the same, and the scan
    // checks every fresh offset against that -- no slot, no copy launch.
    // The same knowledge lets the rows of the register classes (products sorted in registers, nothing sized by the
    // nnz) be finished in the SYMBOLIC phase: one walk of the row instead of two.  The numeric phase then accounts for
    // them as rows that are already in place.
    constexpr u32 kEscNum = kNumEscMask;
    p.fused = c->esc_fused && c->nf_direct && c->pred_valid && (p.num_mask & kEscNum) != 0 &&
              c->cp.sym_g8 == c->cp.num_g8;
    if (p.fused) {
        for (int k = 0; k < kMaxClasses; ++k)
            if (kEscNum >> k & 1u) {
                p.num_counts[NUM_NFCOPY] += p.num_counts[k];
                p.num_counts[k] = 0;
            }
        p.num_mask = (p.num_mask & ~kEscNum) | (1u << NUM_NFCOPY);
    }
    p.direct = c->nf_direct && c->pred_valid && (p.num_mask >> NUM_NFCOPY & 1u);
    p.launch_mask = p.direct ? (p.num_mask & ~(1u << NUM_NFCOPY)) : p.num_mask;
    // Nothing downstream needs what the analysis WRITES when the previous identical call left all of it in the arena:
    // the analysis becomes a verifier beside the sequence (its own stream, its own ticket).
    // (on the library's own pipeline stream only: beside a CALLER's stream the verifier would not be ordered behind the
    //  work that produces the inputs there; rows that take a scratch slot keep the writing analysis)
    p.overlap = c->overlap_analysis && arena_mine && c->pred_valid && c->vstream != nullptr && !c->use_user_stream &&
                !(c->prev.sym_mask >> SYM_GH & 1u) && (!(c->prev.sym_mask >> SYM_NF & 1u) || p.direct) &&
                (p.direct || !(p.num_mask >> NUM_NFCOPY & 1u));
    // ... and when the arena was last written by a replay of THIS sequence, its scan has nothing left to do either: the
    // offsets, classes, records and lists it would produce are a function of the rows' nnz and of the analysis' quantities
    // -- all verified where they are produced.  C.row_offsets is still rewritten in every call (from the sequence's copy
    // of the offsets, by extra workgroups of the numeric light launch: needs that launch).
    // (... or has no rows that are finished early at all: every row then goes through the numeric light launch)
    const bool early_ok = (p.fused && p.direct) || (p.num_mask & (kEscNum | (1u << NUM_NFCOPY))) == 0;
    // In such a sequence the symbolic pass of a hash / dense row has ONE reader left: the comparison of its count with the
    // previous call's.  The numeric bodies can make that comparison themselves (numeric.hip, VERIFY) -- when it PAYS: the
    // verifying bodies cost the numeric light launch 5-15 %, while the symbolic pass of a FEW hash rows beside many
    // register-class rows hides inside the fused launch.  (option num_verify = 2: whenever possible)
    float us_hash = 0.f, us_esc = 0.f;
    for (int k = 0; k < kMaxClasses; ++k)
        ((kSymEscMask >> k & 1u) ? us_esc : us_hash) += p.sym_counts[k] * kSymNsPerRow[k] * 1e-3f;
    const bool want_verify = c->num_verify && (p.fused || !(p.launch_mask & kEscNum)) && !(p.sym_mask >> SYM_NF & 1u) &&
                             (c->num_verify >= 2 || us_hash > us_esc);
    const u32 eff_sym = want_verify ? (p.sym_mask & kSymEscMask) : p.sym_mask;
    p.skip_scan = c->skip_scan && arena_replay_ok && p.overlap && early_ok &&
                  (p.launch_mask & kNumBigLightMask) != 0 && (eff_sym & ~kSymLightMask) == 0;
    p.num_verify = want_verify && p.skip_scan;
    p.safe_numeric = (p.launch_mask & kEscNum) == 0;
    return p;
}

// front + back + ticket of a reuse sequence, straight onto the stream
template <typename T>
int enqueue_replay(speck_config* c, hipStream_t s, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* C,
                   const Scratch& sc, const ReplayPlan& p)
{
    CallForm f;
    f.fused = p.fused, f.direct = p.direct, f.overlap = p.overlap, f.skip_scan = p.skip_scan;
    f.num_verify = p.num_verify || p.safe_numeric;
    // C.row_offsets <- the staged offsets of this call's scan, or (no scan) the sequence's own copy of the offsets
    f.off_src = p.skip_scan ? c->gpred.off : sc.offsets;
    f.off_dst = C->row_offsets;
    f.off_n = (u32)A->rows + 1u;
    f.c_col = C->col_ids, f.c_val = C->data;
    f.nf_wcols = p.nf_wcols;  // (the plan's, not the config's: another problem may have been analysed since)
    // (num_verify: the symbolic phase is the register classes alone -- the plan keeps every class, for the form of the
    //  sequence that runs when the arena is not this problem's)
    u32 sym_counts[kMaxClasses];
    std::memcpy(sym_counts, p.sym_counts, sizeof(sym_counts));
    FrontArgs a;
    a.exact_nnz = C->nnz;
    a.sym_mask = p.sym_mask, a.num_mask = p.num_mask, a.sym_hint = sym_counts;
    a.expect_g = p.g_products, a.expect_g_rows = p.num_counts[NUM_G], a.expect_nf = p.nf_cap_entries;
    if (p.num_verify) {
        a.sym_mask &= kSymEscMask;
        for (int k = 0; k < kMaxClasses; ++k)
            if (!(kSymEscMask >> k & 1u)) sym_counts[k] = 0;
    }
    int rc = enqueue_front(c, s, A, B, sc, (u32)sizeof(T), f, a, nullptr);
    if (rc != SPECK_OK) return rc;
    rc = enqueue_back<T>(c, s, A, B, sc, f, C->col_ids, static_cast<T*>(C->data), p.launch_mask, p.num_counts, nullptr);
    if (rc != SPECK_OK) return rc;
    // the last kernel mirrors the (final) statistics block into pinned host memory, then stores the completion ticket
    launch_done(s, c->d_ticket, c->h_ticket_dev, c->d_stats, c->h_stats_dev);
    return SPECK_OK;
}

// per-launch / per-phase times of the last call from its events (speck_stats)
void publish_kernel_times(speck_config* c, const Timing& tm, size_t ev_num_end)
{
    auto ms = [&](size_t a) {
        float v = 0.f;
        (void)hipEventElapsedTime(&v, c->kev[a], c->kev[a + 1]);
        return v;
    };
    (void)hipEventElapsedTime(&c->last.analysis_ms, c->kev[tm.ev_analysis], c->kev[tm.ev_analysis_end]);
    c->last.scan_ms = ms(tm.ev_scan);
    // phases: end of the analysis launch -> start of the scan (all symbolic branches joined);
    // before the first numeric launch -> after the last join
    (void)hipEventElapsedTime(&c->last.sym_phase_ms, c->kev[tm.ev_analysis_end], c->kev[tm.ev_scan]);
    (void)hipEventElapsedTime(&c->last.num_phase_ms, c->kev[tm.ev_num], c->kev[ev_num_end]);
    for (const auto& ct : tm.sym) {
        if (ct.cls == kLight) c->last.sym_light_ms = ms(ct.ev);
        else c->last.sym_bin_ms[ct.cls] = ms(ct.ev);
    }
    for (const auto& ct : tm.num) {
        if (ct.cls == kLight) c->last.num_light_ms = ms(ct.ev);
        else c->last.num_bin_ms[ct.cls] = ms(ct.ev);
    }
    c->last.kernel_events_valid = 1;
}

// The analysis of a reuse sequence as a VERIFIER (ReplayPlan::overlap): on its own stream, enqueued by the host
// right behind the sequence, so that it runs beside it.  It compares what it computes from A and B as they are now with
// what the previous identical call left in the arena -- which is what the sequence's kernels read -- and reports to
// pinned host memory.  wait_verifier: the verdict, once that stream is idle (it is, long before the sequence's ticket).
int launch_verifier(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, const Scratch& sc)
{
    __atomic_store_n(c->h_verify, 0u, __ATOMIC_RELEASE);
    c->verifier_in_flight = true;
    // The interior of B's rows is no input of the analysis, and nothing the sequence's own checks compare (a row's nnz,
    // its place in C) tells a row whose ids were reordered in place from a sorted one: the precondition of EVERY call is
    // checked with the call -- one streaming pass over B.col_ids on this stream; a violation voids the sequence like any
    // other change and the complete call that re-runs reports it (SPECK_ERR_UNSORTED).
    auto validate = [&] {
        if (c->validate_inputs)
            launch_validate_b(c->vstream, B->row_offsets, B->col_ids, (u32)B->rows, (u32)B->cols, B->nnz, c->h_verify_dev);
    };
    if (c->verify_inputs && c->snap && c->snap_for_arena) {
        // the arena's metadata is a function of inputs that are still what the writing analysis saw: four streams compared
        launch_verify_inputs(c->vstream, A->row_offsets, sc.a_ro_copy, (u32)A->rows, A->col_ids, c->snap, A->nnz, B->row_offsets,
                             B->col_ids, (u32)B->rows, c->snap + c->snap_a_words, c->h_verify_dev);
        validate();
        launch_ticket(c->vstream, c->d_vticket, c->h_verify_dev + 16);
        LAUNCHES_OK();
        return SPECK_OK;
    }
    ClassifyParams cp = c->cp;
    cp.sym_allowed = cp.num_allowed = 0xFFFFFFFFu;
    cp.esc16 = (c->cp.esc16 && B->cols <= (1ull << 26)) ? 1u : 0u;  // (as enqueue_front classifies)
    cp.esc_fused = 0;
    launch_analysis(c->vstream, A->row_offsets, A->col_ids, B->row_offsets, B->col_ids, (u32)A->rows, A->nnz, sc.row_ops,
                    sc.row_max_ops, sc.row_col_min, sc.row_col_max, sc.cls_sym, sc.counts, sc.sym_recs, c->d_stats, cp,
                    sc.b_sl, Chain{nullptr, nullptr, nullptr, 0u, ~0u}, sc.nf_off, ~0ull, (u32)B->rows, sc.a_ro_copy, c->h_verify_dev, nullptr, B->nnz);
    // ... and behind it the copy of the inputs it has just verified the arena against (they do not change while the call
    // is in flight): the verifiers of the next replays compare with that.
    if (c->verify_inputs && c->snap) {
        launch_snapshot_inputs(c->vstream, A->row_offsets, A->col_ids, c->snap, A->nnz, B->row_offsets, B->col_ids, (u32)B->rows,
                               c->snap + c->snap_a_words);
        c->snap_pending = true;
    }
    validate();
    launch_ticket(c->vstream, c->d_vticket, c->h_verify_dev + 16);
    LAUNCHES_OK();
    return SPECK_OK;
}
int wait_verifier(speck_config* c, bool* changed)
{
    // (the verifier finishes long before the sequence: by the time the host looks its ticket is there -- no API call)
    const u32 want = ++c->vticket_expected;
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    while (!(seen = __atomic_load_n(c->h_verify + 16, __ATOMIC_ACQUIRE) == want)) {
        for (int i = 0; i < 64; ++i) cpu_relax();
        if (std::chrono::steady_clock::now() - t0 > kSpinBudget) break;
    }
    if (!seen) HIP_TRY(hipStreamSynchronize(c->vstream));
    c->vticket_expected = __atomic_load_n(c->h_verify + 16, __ATOMIC_ACQUIRE);
    c->verifier_in_flight = false;
    *changed = __atomic_load_n(c->h_verify, __ATOMIC_ACQUIRE) != 0u;
    return SPECK_OK;
}
// No way out of a call leaves work on the verifier's stream: the next call zeroes the verdict word and counts tickets
// (an early return between launch_verifier and wait_verifier let an orphaned verifier OR into the next
// call's verdict).
struct VerifierGuard {
    speck_config* c;
    ~VerifierGuard()
    {
        if (!c->verifier_in_flight) return;
        (void)hipStreamSynchronize(c->vstream);
        c->vticket_expected = __atomic_load_n(c->h_verify + 16, __ATOMIC_ACQUIRE);
        c->verifier_in_flight = false;
        c->validate_in_flight = false;
    }
};

// The input check of a complete call, beside it on the verifier's stream (stages.hip: validate_b_kernel).
int begin_validate(speck_config* c, const speck_dcsr* B, hipStream_t gate)
{
    __atomic_store_n(c->h_verify, 0u, __ATOMIC_RELEASE);
    if (c->use_user_stream) {
        // the caller's stream may still be producing B: the check goes behind what is queued there now
        HIP_TRY(hipEventRecord(c->fork, c->user_stream));
        HIP_TRY(hipStreamWaitEvent(c->vstream, c->fork, 0));
    }
    c->verifier_in_flight = true;
    // A large B: the check is a stream of nnz(B) column ids, the analysis it would run beside is bound by the same
    // bandwidth and heads the call's critical path -- the check starts BEHIND it, beside the symbolic launches (bound by
    // instruction issue).  (`gate`: the stream the analysis was just enqueued on)
    if (gate && B->nnz >= c->validate_after_nnz) {
        HIP_TRY(hipEventRecord(c->vgate, gate));
        HIP_TRY(hipStreamWaitEvent(c->vstream, c->vgate, 0));
    }
    launch_validate_b(c->vstream, B->row_offsets, B->col_ids, (u32)B->rows, (u32)B->cols, B->nnz, c->h_verify_dev);
    launch_ticket(c->vstream, c->d_vticket, c->h_verify_dev + 16);
    LAUNCHES_OK();
    c->validate_in_flight = true;
    return SPECK_OK;
}
// ... its verdict (waits for the check if it is still running: it is not, by the time anybody asks)
int finish_validate(speck_config* c, bool* b_invalid)
{
    *b_invalid = false;
    if (!c->validate_in_flight) return SPECK_OK;
    c->validate_in_flight = false;
    bool any = false;
    const int rc = wait_verifier(c, &any);
    if (rc != SPECK_OK) return rc;
    *b_invalid = (__atomic_load_n(c->h_verify, __ATOMIC_ACQUIRE) & 4u) != 0;
    return SPECK_OK;
}
// What a complete call says of its inputs once the statistics of a batch are on the host: A (the analysis checks its
// column ids), then B (the input check)
int input_verdict(speck_config* c)
{
    if (c->h_stats->a_invalid) return SPECK_ERR_INVALID;
    bool b_bad = false;
    const int rc = finish_validate(c, &b_bad);
    if (rc != SPECK_OK) return rc;
    return b_bad ? SPECK_ERR_UNSORTED : SPECK_OK;
}
// A batch that wrote into the caller's buffers on the strength of the previous complete call: did that hold?
bool speculation_held(const DeviceStats* h, u64 nnz_c)
{
    return !h->capacity_miss && !h->nnz_overflow && h->nnz_c == nnz_c && h->sum_products != 0;
}
// The sizing hints of such a batch: the rows per symbolic class of the previous complete call; returns the classes it
// launches.  (The light launch is one kernel whatever it holds: every class of it may have rows.)
u32 speculated_hints(const speck_config* c, u32 (&hints)[kMaxClasses])
{
    u32 mask = kSymLightMask;
    for (int k = 0; k < kMaxClasses; ++k) {
        hints[k] = c->prev.sym_counts[k];
        if (hints[k]) mask |= 1u << k;
        if ((kSymLightMask >> k & 1u) && !hints[k]) hints[k] = 256;
    }
    return mask;
}

// How an attempt at one kind of call ended, beside its status code
enum class Attempt {
    not_tried,     // its conditions do not hold: nothing was enqueued
    done,          // the call is complete
    missed,        // the device objected and nothing of C was written: the next kind starts over
    front_stands,  // through call only: the scan alone objected -- analysis .. scan stand, the call goes on behind them
};

// One multiply in flight: what every kind of call needs.  Built on the stack by multiply_impl and gone with the call --
// with it the row offsets the call allocated, unless C has taken them.  The kinds are tried in the order of the
// declarations below (multiply_impl).
template <typename T>
struct Call {
    speck_config* const c;
    const speck_dcsr *const A, *const B;
    speck_dcsr* const C;
    speck_timings* const t;
    const hipStream_t s;
    const u32 m;
    Scratch sc{};
    // The input check -- B's rows strictly ascending and in range: one coalesced pass over B.col_ids -- runs BESIDE the
    // call on the verifier's stream; its verdict is looked at with the statistics of the scan, before anything of C is
    // written.  Until then the kernels stay inside their tables and windows whatever B holds (a requirement for every
    // kernel body: DESIGN.md 1).  A's column ids are checked -- and clamped -- by the analysis.
    // (launched BEHIND the analysis of the call, not in front of it: enqueue_front starts it)
    InputCheck check;
    Timing tm;
    StageTimer st;
    const bool c_ready;        // C holds buffers for a product of A's row count
    // what this call leaves behind for a repeated identical call: its row offsets, written by the scan kernel next to its
    // other outputs.  No room on the device: that call places nothing early.
    bool keep_pred = false;
    u32* pred_out = nullptr;
    bool early_stats = false;  // the scan mirrors the statistics and stores the ticket itself: await_scan_stats
    u32 num_mask = 0;          // numeric classes with rows, once the host knows them
    size_t ev_num_end = 0;
    u32* c_ro = nullptr;       // the row offsets of C ...
    bool own_ro = false;       // ... allocated by this call and not yet C's

    Call(speck_config* c_, const speck_dcsr* A_, const speck_dcsr* B_, speck_dcsr* C_, speck_timings* t_, hipStream_t s_)
        : c(c_), A(A_), B(B_), C(C_), t(t_), s(s_), m((u32)A_->rows), check{c_, B_, s_}, st(c_, t_->measureAll != 0, s_),
          c_ready(C_->rows == A_->rows && C_->row_offsets && C_->col_ids && C_->data && C_->nnz > 0) {}
    ~Call() { if (own_ro) (void)guarded_free(c_ro); }
    // C holds usable buffers whose size fits 32 bits: an attempt may write the product into them
    bool c_usable() const { return c_ready && C->nnz <= 0xFFFFFFFFull; }
    // a form of this call: the config's numeric-first window as it is NOW, the input check behind the analysis
    CallForm form()
    {
        CallForm f;
        f.nf_wcols = c->nf_wcols, f.after_analysis = &check;
        return f;
    }
    int front(const CallForm& f, const FrontArgs& a) { return enqueue_front(c, s, A, B, sc, (u32)sizeof(T), f, a, &tm); }
    int back(const CallForm& f, u32* c_col, void* c_val, u32 mask, const u32* counts)
    {
        return enqueue_back<T>(c, s, A, B, sc, f, c_col, static_cast<T*>(c_val), mask, counts, &tm);
    }
    // parts of the front of a plain two-phase call (the offsets go to scratch: C.row_offsets -- possibly the caller's
    // reused buffer -- is written only once nothing can fail any more)
    int plain_front(u32 parts, const u32* sym_known)
    {
        FrontArgs a;
        a.parts = parts, a.sym_hint = parts == 2u ? sym_known : nullptr;
        a.host_mirror = early_stats ? c->h_stats_dev : nullptr, a.pred_off_out = pred_out;
        return front(form(), a);
    }
    // the statistics of a front's scan on the host, then what the call says of its inputs
    int await_front() { const int rc = early_stats ? await_scan_stats(c, s) : read_stats(c, s); return rc == SPECK_OK ? input_verdict(c) : rc; }
    // the numeric launches of a call between their two profiling events
    template <typename F>
    int timed_numeric(F&& enqueue)
    {
        if (c->profile_kernels) {
            tm.ev_num = tm.ev;
            (void)hipEventRecord(kernel_event(c, tm.ev++), s);
        }
        const int rc = enqueue();
        if (rc != SPECK_OK) return rc;
        ev_num_end = tm.ev;
        if (c->profile_kernels) (void)hipEventRecord(kernel_event(c, tm.ev++), s);
        return SPECK_OK;
    }
    // The settle step of a batch that wrote into the caller's buffers on the strength of the previous complete call: the
    // statistics (done_kernel + ticket: the one wait of the call), the verdict on the inputs (a B that fails the check:
    // the device saw the verdict, nothing of C was written), whether the speculation held -- counted
    int settle_batch(int& hits, int& misses, bool* held)
    {
        int rc = read_stats(c, s);
        if (rc == SPECK_OK) rc = input_verdict(c);
        if (rc != SPECK_OK) return rc;
        *held = speculation_held(c->h_stats, C->nnz);
        ++(*held ? hits : misses);
        return SPECK_OK;
    }
    // this attempt missed: the next one checks B again (the verdict word of the check was consumed)
    int miss(Attempt& how, bool forget_events)
    {
        check.started = false;
        if (forget_events) tm = Timing{};
        how = Attempt::missed;
        return SPECK_OK;
    }
    int finish_complete()
    {
        if (t->measureCompleteTime) {
            // reference: cudaDeviceSynchronize + complete event, Multiply.cu:1082-1085
            HIP_TRY(hipEventRecord(c->completeEnd, s));
            HIP_TRY(hipEventSynchronize(c->completeEnd));
            HIP_TRY(hipEventElapsedTime(&t->complete, c->completeStart, c->completeEnd));
        }
        return SPECK_OK;
    }

    // ---- REUSE sequence (option "reuse").  Applies when C is allocated and nothing is being timed; runs when the call has the
    // buffers of the previous call and C holds the expected nnz: the sequence that places rows where that call put them
    // (plan_replay).  The device checks every assumption; on a miss the complete call re-runs.
    int try_replay(Attempt& how)
    {
        if (!c->reuse || !c_ready || c->profile_kernels || t->measureAll) return SPECK_OK;
        const CallKey key = make_key<T>(c, A, B, C, s);
        const bool arena_mine = c->arena_key_valid && c->arena_key == key;
        const bool replay_layout = arena_mine && c->arena_from_replay;
        bool have = c->plan_valid && c->plan_key == key;
        // a new sequence: behind a complete call of this problem; again once it has replayed (no scan from then on)
        if ((!have || (!c->plan.skip_scan && replay_layout)) && c->last_key_valid && c->last_key == key) {
            if (!have && snapshot_prediction(c, s) != SPECK_OK) c->pred_valid = false;  // (no room: nothing is placed early)
            c->plan = plan_replay(c, true, replay_layout);
            c->plan_key = key;
            c->plan_valid = have = true;
            ++c->plans_made;
        }
        if (!have) return SPECK_OK;
        // A sequence whose analysis only VERIFIES reads the metadata the previous multiply of THIS problem left in the
        // arena.  If something else has used the arena since (another problem on this config, a stage entry point) the
        // same sequence runs with a writing analysis in front instead and leaves the arena as the next replay needs it.
        ReplayPlan p = c->plan;
        if ((p.overlap && !arena_mine) || (p.skip_scan && !replay_layout)) p.overlap = p.skip_scan = p.num_verify = false;
        c->arena_key_valid = false;  // (until this call has completed)
        auto missed = [&] {  // inputs changed under the same pointers: the complete call re-runs
            ++c->replay_misses;
            drop_plan(c);
            how = Attempt::missed;
            return SPECK_OK;
        };
        // (a sequence with its own analysis: the input check of B alone, beside it from its first launch on; one whose
        //  numeric launches are the plain forms: the check FIRST -- they must not see a B that fails it)
        bool b_first_bad = false, changed = false;
        int rc = SPECK_OK;
        if (!p.safe_numeric && !p.num_verify && c->validate_inputs) {
            rc = begin_validate(c, B);
            if (rc == SPECK_OK) rc = finish_validate(c, &b_first_bad);
        } else if (!p.overlap && c->validate_inputs) {
            rc = begin_validate(c, B);
        }
        if (rc != SPECK_OK) return rc;
        if (b_first_bad) return missed();
        rc = enqueue_replay<T>(c, s, A, B, C, sc, p);
        // (the verifier behind the sequence, while it runs: the host would only spin otherwise)
        if (rc == SPECK_OK && p.overlap) rc = launch_verifier(c, A, B, sc);
        // the last kernel of the sequence stores a ticket into pinned memory
        if (rc == SPECK_OK) rc = wait_ticket(c, s);
        if (rc == SPECK_OK) rc = p.overlap ? wait_verifier(c, &changed) : finish_validate(c, &changed);
        if (rc != SPECK_OK) return rc;
        if (c->h_stats->chain_error) return chain_failed(c, s);
        if (changed || c->h_stats->capacity_miss || c->h_stats->nnz_overflow || c->h_stats->nnz_c != C->nnz) return missed();
        c->arena_key = key;
        c->arena_key_valid = c->arena_from_replay = true;
        if (c->snap_pending) c->snap_for_arena = true;  // (the copy of the inputs this call's verifier took)
        ++c->replays;
        publish_counts(c, s);
        c->last.replayed = 1;
        c->last.nf_direct = p.direct ? 1 : 0, c->last.esc_fused = p.fused ? 1 : 0;
        // bits 0-1: rows are placed by / compared with the previous call's offsets (the sequence's own copy); 2: the analysis only
        // verifies, beside the sequence; 3: no scan kernel; 4: no symbolic pass for the hash / dense rows
        c->last.pred_stages = (c->pred_valid ? 3 : 0) | (p.overlap ? 4 : 0) | (p.skip_scan ? 8 : 0) | (p.num_verify ? 16 : 0);
        how = Attempt::done;
        return finish_complete();
    }

    // ---- COMPLETE call: the arena is rewritten (it is this problem's once the call has completed), the row offsets of C by
    // the reuse rule of the reference (INIT, Multiply.cu:156-165), what the call will leave for a repeated identical one
    int begin_complete()
    {
        c->arena_key_valid = false;
        if (C->rows == A->rows && C->row_offsets != nullptr) {
            c_ro = C->row_offsets;
        } else {
            HIP_TRY(guarded_malloc(reinterpret_cast<void**>(&c_ro), (size_t(m) + 1) * sizeof(u32)));
            own_ro = true;
        }
        t->init = st.lap();
        c->pred_valid = false;
        keep_pred = c->nf_direct && c->reuse && ensure_pred(c->pred, m);
        early_stats = c->spin_wait && !c->profile_kernels;
        pred_out = keep_pred ? c->pred.off : nullptr;
        return SPECK_OK;
    }

    // ---- HASH ONE-WALK call (walk_hash_kernel, numeric.hip; option one_walk_hash): analysis -> walk_hash_kernel -> done.
    // Applies when C is allocated and the previous complete call, of the same shapes, says that every row fits the sub-wave
    // hash table -- longest row of C within the 256-entry class, most rows hash rows; checked row by row on the device.
    int try_walk_hash(Attempt& how)
    {
        const LastCall& prev = c->prev;
        const u32* sl = prev.sym_counts;
        const u64 hash_rows = u64(sl[SYM_W128]) + sl[SYM_W256] + sl[SYM_W1K];
        const u64 groups = (u64(m) + kWalkHashRows - 1) / kWalkHashRows;
        const bool pays = c->one_walk_hash >= 2 || 2 * hash_rows >= m;
        if (!c->one_walk_hash || !pays || !c_usable() || !prev.ran_on(A, B) || c->use_user_stream || prev.max_row_nnz == 0 ||
            prev.max_row_nnz > kNumW256MaxNnz || prev.max_row_ops > 4096 || groups > kChain3MaxGroups)
            return SPECK_OK;
        Chain3 ch3;
        int rc = next_chain3(c, s, groups, &ch3);
        if (rc != SPECK_OK) return rc;
        FrontArgs fa;
        fa.parts = 1u;
        rc = front(form(), fa);
        if (rc != SPECK_OK) return rc;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (c->profile_kernels) {
            tm.ev_scan = tm.ev;
            e0 = kernel_event(c, tm.ev++);
            e1 = kernel_event(c, tm.ev++);
        }
        WalkHashArgs wa{};
        wa.a_ro = A->row_offsets, wa.m = m, wa.max_ops = 4096, wa.vsize = (u32)sizeof(T);
        wa.row_ops = sc.row_ops, wa.row_col_min = sc.row_col_min, wa.row_col_max = sc.row_col_max;
        wa.offsets_out = sc.offsets, wa.pred_off_out = nullptr, wa.st = c->d_stats;
        wa.c_col = C->col_ids, wa.c_val = C->data, wa.c_cap = C->nnz;
        wa.want_bytes = c->cp.want_bytes, wa.bytes_acc = c->cp.want_bytes ? c->d_bytes : nullptr;
        wa.debug = c->walk_hash_debug;
        const ProductSrc<T> src{sc.b_sl, static_cast<const T*>(A->data), B->col_ids, static_cast<const T*>(B->data), sc.w_sl};
        launch_walk_hash<T>(s, wa, src, ch3, e0, e1);
        (void)timed_numeric([&] {
            launch_copy_offsets(s, sc.offsets, C->row_offsets, m + 1, c->d_stats);
            return SPECK_OK;
        });
        LAUNCHES_OK();
        bool held = false;
        rc = settle_batch(c->walks, c->walk_misses, &held);
        if (rc != SPECK_OK) return rc;
        if (!held) return miss(how, true);
        publish_counts(c, s);
        c->last.one_walk = 2;
        c->last.num_bin_rows[NUM_W256] = m;  // (every row went through the 256-entry sub-wave body)
        t->spGEMMCounting = 0.f;
        t->spGEMMNumeric = st.lap();
        // the arena holds no numeric records / lists of this call: a reuse sequence is planned from a two-phase
        // call only; the figures this path was chosen by are refreshed
        c->prev.max_row_nnz = c->h_stats->max_row_nnz_c, c->prev.max_row_ops = c->h_stats->max_row_ops;
        c->last_key_valid = c->arena_key_valid = c->pred_valid = false;
        drop_plan(c);
        how = Attempt::done;
        rc = finish_complete();
        if (rc != SPECK_OK) return rc;
        if (c->profile_kernels) {
            HIP_TRY(hipStreamSynchronize(s));
            publish_kernel_times(c, tm, ev_num_end);
        }
        return SPECK_OK;
    }

    // ---- ONE-WALK call (walk.hip; option one_walk).  Applies when C is allocated and a complete call of the same shapes has
    // run on the config: the rows of the register classes are finished in ONE walk inside the kernel that places the rows --
    // no symbolic pass for them, no scan kernel, no read-back before the numeric launches.  Everything the sequence assumes
    // (classes with rows, pool and buffer sizes, nnz(C) = what the caller's buffers hold) is checked on the device; on a miss
    // the two-phase call re-runs (and re-allocates C as the reference does when nnz changes, Multiply.cu:589-592).
    int try_one_walk(Attempt& how)
    {
        const LastCall& prev = c->prev;
        if (!c->one_walk || !c_usable() || !prev.ran_on(A, B) || m > walk_max_rows() || c->use_user_stream) return SPECK_OK;
        const u32* sl = prev.sym_counts;
        const u64 esc_rows = u64(sl[SYM_G8]) + sl[SYM_G16] + sl[SYM_R32] + sl[SYM_R64];
        const u64 esc_bound = 32ull * sl[SYM_G8] + 64ull * sl[SYM_G16] + 128ull * sl[SYM_R32] + 256ull * sl[SYM_R64];
        // it pays when the rows the walk kernel finishes (or moves) are a good share of all rows
        const bool pays = c->one_walk >= 2 || 8 * (esc_rows + sl[SYM_NF]) >= m;
        const u64 want = prev.was_walk ? prev.nf_entries + prev.nf_entries / 32 + 4096 : prev.nf_entries + esc_bound + 4096;
        if (!pays || want >= (1ull << 40) || ensure_nfpool(c, want, sizeof(T)) != SPECK_OK) return SPECK_OK;
        u32 hints[kMaxClasses];
        const u32 launch_mask = prev.num_mask & ~(kNumEscMask | (1u << NUM_NFCOPY));
        CallForm f = form();
        f.one_walk = true;
        f.c_col = C->col_ids, f.c_val = C->data, f.c_cap = C->nnz;
        f.off_src = sc.offsets, f.off_dst = C->row_offsets, f.off_n = m + 1;
        FrontArgs fa;
        fa.sym_mask = speculated_hints(c, hints) & ~kSymEscMask, fa.num_mask = launch_mask;
        fa.sym_hint = hints, fa.hint_exact = false;
        fa.expect_g = prev.g_products, fa.expect_g_rows = prev.num_counts[NUM_G], fa.expect_nf = c->nf_cap_entries;
        fa.pred_off_out = pred_out;
        int rc = front(f, fa);
        if (rc != SPECK_OK) return rc;
        rc = timed_numeric([&] { return back(f, C->col_ids, C->data, launch_mask, prev.num_counts); });
        if (rc != SPECK_OK) return rc;
        bool held = false;
        rc = settle_batch(c->walks, c->walk_misses, &held);
        if (rc != SPECK_OK) return rc;
        if (!held) return miss(how, false);  // (unlike the other two misses this one has never forgotten the attempt's events: kept)
        publish_counts(c, s);
        num_mask = mask_of(c->h_stats->num.count, NUM_CLASSES);
        c->last.one_walk = 1;
        t->spGEMMCounting = 0.f;
        t->spGEMMNumeric = st.lap();
        how = Attempt::done;
        return SPECK_OK;
    }

    // ---- THROUGH call (option eager_through): a complete two-phase call enqueued in ONE batch -- analysis, symbolic, scan AND
    // the numeric launches, sized from the previous complete call on this config.  Applies when that call had the same shapes
    // and was no walk, C holds buffers of the size it produced, and nothing is being timed or counted.  What the host checks
    // between the two phases of a two-phase call the scan checks on the device; a miss leaves C untouched.
    int try_through(Attempt& how)
    {
        const LastCall& prev = c->prev;
        if (!c->eager_through || !c->eager_speculate || !prev.ran_on(A, B) || !c_usable() || C->nnz != prev.eager_stats.nnz_c ||
            !prev.num_mask || prev.was_walk || c->profile_kernels || t->measureAll || !c->spin_wait || c->cp.want_bytes ||
            ((prev.num_mask >> NUM_G & 1u) && c->spill.plan == nullptr))
            return SPECK_OK;
        u32 hints[kMaxClasses];
        CallForm f = form();
        f.through_gate = c->validate_inputs ? c->h_verify_dev : nullptr;
        // (the ticket the check of THIS call will store: wait_verifier counts them)
        f.through_ticket = (c->validate_inputs && B->nnz < c->validate_after_nnz) ? c->vticket_expected + 1u : 0u;
        f.off_src = sc.offsets, f.off_dst = C->row_offsets, f.off_n = m + 1;  // (c_ready: c_ro IS C's array)
        FrontArgs fa;
        fa.exact_nnz = C->nnz;
        fa.sym_mask = speculated_hints(c, hints), fa.num_mask = prev.num_mask, fa.sym_hint = hints;
        if (prev.num_mask >> NUM_G & 1u) fa.expect_g = prev.g_products, fa.expect_g_rows = prev.num_counts[NUM_G];
        fa.expect_nf = c->nf_cap_entries, fa.pred_off_out = pred_out;
        int rc = front(f, fa);
        if (rc == SPECK_OK) rc = back(f, C->col_ids, C->data, prev.num_mask, prev.num_counts);
        bool held = false;
        if (rc == SPECK_OK) rc = settle_batch(c->through_hits, c->through_misses, &held);
        if (rc != SPECK_OK) return rc;
        if (held) {
            publish_counts(c, s);
            num_mask = mask_of(c->h_stats->num.count, NUM_CLASSES);
            c->prev.g_products = c->h_stats->g_products;
            c->last.eager_speculated = c->last.eager_through = 1;
            t->countProducts = t->loadBalanceCounting = t->globalMapsCounting = t->globalMapsNumeric = t->allocC = t->loadBalanceNumeric = 0.f;
            t->spGEMMCounting = 0.f;
            t->spGEMMNumeric = st.lap();
            how = Attempt::done;
        } else if (!c->h_stats->front_miss && !c->h_stats->nnz_overflow) {
            // only the scan objected (another nnz(C), a numeric class without a launch, the spill pool): its offsets, counts
            // and class lists stand -- the call goes on behind its ONE read-back like a speculated call whose checks held;
            // the numeric launches queued above found the flag and wrote nothing
            HIP_TRY(hipMemsetAsync(&c->d_stats->capacity_miss, 0, sizeof(u32), s));
            c->h_stats->capacity_miss = 0;
            how = Attempt::front_stands;
        } else
            return miss(how, true);
        return SPECK_OK;
    }

    // ---- SPECULATED batch (option eager_speculate): analysis .. scan as ONE batch, sized from the previous complete call on
    // this config when it had the same shapes: the classes that call had rows in (a row in any other class raises
    // capacity_miss), grids from its counts, its scratch pool and numeric-first window (checked by the analysis /
    // numeric-first kernels).  Saves the first of the two read-backs; *held: the front stands.
    int front_speculated(bool* held)
    {
        if (!c->eager_speculate || !c->prev.ran_on(A, B)) return SPECK_OK;
        u32 spec_counts[kMaxClasses];
        FrontArgs fa;
        fa.sym_mask = speculated_hints(c, spec_counts), fa.sym_hint = spec_counts;
        fa.host_mirror = early_stats ? c->h_stats_dev : nullptr;
        fa.expect_nf = c->nf_cap_entries, fa.pred_off_out = pred_out;
        int rc = front(form(), fa);
        if (rc == SPECK_OK) rc = await_front();
        if (rc != SPECK_OK) return rc;
        *held = !c->h_stats->capacity_miss;
        ++(*held ? c->eager_spec_hits : c->eager_spec_misses);
        c->last.eager_speculated = *held ? 1 : -1;
        return SPECK_OK;
    }

    // ---- the front of the plain TWO-PHASE call: ANALYSIS + binning, SYMBOLIC + SCAN (Multiply.cu:239-575) -- one read-back,
    // two when a scratch-pool class is on
    int front_two_phase()
    {
        u32 sym_now[kMaxClasses];
        const u32* sym_known = nullptr;  // rows per symbolic class, once a read-back of this call has them
        int rc = plain_front(1u, nullptr);
        if (rc != SPECK_OK) return rc;
        if (c->cp.nf_min_ops || c->cp.gh_per_window) {
            // numeric-first rows (and the global key sets of SYM_GH rows) need their scratch pool before the
            // symbolic phase: one more read-back
            rc = read_stats(c, s);
            if (rc != SPECK_OK) return rc;
            if (c->h_stats->a_invalid) return SPECK_ERR_INVALID;
            // No room (or no budget) for the pool: first the global key sets go (those rows take the multi-window
            // bitmap, which needs no memory), then the numeric-first rows (they take the two-phase path) -- for this
            // config from now on; the rows are classified again.
            while (c->h_stats->nf_entries) {
                rc = ensure_nfpool(c, c->h_stats->nf_entries, sizeof(T));
                if (rc != SPECK_ERR_OOM) break;
                if (c->cp.gh_per_window && c->h_stats->sym.count[SYM_GH]) c->cp.gh_per_window = 0;
                else if (c->cp.nf_min_ops && c->h_stats->sym.count[SYM_NF]) c->cp.nf_min_ops = 0;
                else break;
                ++c->pool_fallbacks;
                rc = plain_front(1u, nullptr);
                if (rc == SPECK_OK) rc = read_stats(c, s);
                if (rc != SPECK_OK) break;
            }
            if (rc != SPECK_OK) return rc;
            c->nf_wcols = c->h_stats->nf_max_range ? c->h_stats->nf_max_range : kNumD1Cols;
            // the read-back also buys right-sized grids, fork decisions and exact class counts for the symbolic launches
            std::memcpy(sym_now, c->h_stats->sym.count, sizeof(sym_now));
            sym_known = sym_now;
        }
        // (with both scratch-pool classes off the symbolic kernels run before the host has seen the verdict of the
        //  check: they stay inside their tables and windows whatever B holds, and nothing of C is written before the
        //  read-back below)
        rc = plain_front(2u, sym_known);
        return rc == SPECK_OK ? await_front() : rc;
    }

    // ... whichever front stands, its statistics are on the host: the stage times, the counts, and the product without an
    // entry (*empty: C is published with nnz 0 and the call is over)
    int settle_front(bool* empty)
    {
        t->countProducts = t->loadBalanceCounting = t->globalMapsCounting = 0.f;
        t->spGEMMCounting = st.lap();  // analysis + binning + symbolic + scan are one async batch
        publish_counts(c, s);
        if (c->h_stats->nnz_overflow) return SPECK_ERR_NNZ_OVERFLOW;
        *empty = c->h_stats->sum_products == 0;
        if (!*empty) return SPECK_OK;
        // reference: Multiply.cu:256-261 -> matOut.alloc(rows, cols, 0, false)
        if (own_ro) (void)guarded_free(c_ro);
        own_ro = false;
        speck_dcsr_free(C);
        C->rows = A->rows, C->cols = B->cols, C->nnz = 0;
        c->last_key_valid = false;
        return finish_complete();
    }

    // Spill pool of the NUM_G rows FIRST: every failure up to here leaves C untouched (header contract).
    int size_spill_pool()
    {
        num_mask = mask_of(c->h_stats->num.count, NUM_CLASSES);
        if (num_mask >> NUM_G & 1u) {
            // global-memory spill buffers of the heavy rows (role of the reference's global maps,
            // Multiply.cu:357-427), grow-only: per-row plan, per-bucket counters, and two product
            // pools sized from the EXACT product count of the NUM_G rows (numeric.hip, NUM_G)
            const u64 pg = c->h_stats->g_products;
            const u32 rows_g = c->h_stats->num.count[NUM_G];
            const u64 buckets = pg / kGBucketTarget + rows_g + 16;
            const u64 cells = u64(kGCellsPerBucket) * buckets;
            if (cells > 0x7FFFFFFFull) return SPECK_ERR_OOM;
            const size_t need = Carver::need(rows_g, sizeof(GRowPlan)) + Carver::need(cells + 3 * buckets + 4, 4) +
                                Carver::need(buckets, 8) +
                                Carver::need(cells, 4) + Carver::need(buckets, 8) + 2 * Carver::need(buckets, 4) +
                                2 * Carver::need(pg, 4) + 2 * Carver::need(pg, sizeof(T)) + 4096;
            if (need > c->gpool_bytes) {
                drop_plan(c);
                if (c->gpool) (void)guarded_free(c->gpool);
                c->gpool = nullptr, c->gpool_bytes = 0;
                if (guarded_malloc(&c->gpool, need + need / 8) != hipSuccess) {
                    (void)hipGetLastError();
                    return SPECK_ERR_OOM;
                }
                c->gpool_bytes = need + need / 8;
            }
            c->gpool_zones.clear();
            Carver cv(c->gpool, guard_bytes(), &c->gpool_zones);
            SpillBuffers sp{};
            sp.plan = cv.take<GRowPlan>(rows_g);
            // fcount | bcount | bcursor | dcount are cleared by ONE memset: keep them back to back
            u32* counters = cv.take<u32>(cells + 3 * buckets + 4);
            sp.fcount = counters, sp.bcount = counters + cells;
            sp.bcursor = sp.bcount + buckets, sp.dcount = sp.bcursor + buckets, sp.big_count = sp.dcount + buckets;
            sp.big_list = cv.take<u64>(buckets);
            sp.fmap = cv.take<u32>(cells);
            sp.bstart = cv.take<u64>(buckets);
            sp.clo = cv.take<u32>(buckets), sp.chi = cv.take<u32>(buckets);
            sp.pcol[0] = cv.take<u32>(pg), sp.pcol[1] = cv.take<u32>(pg);
            sp.pval[0] = cv.take<T>(pg), sp.pval[1] = cv.take<T>(pg);
            sp.bucket_cap = (u32)buckets, sp.cell_cap = (u32)cells;
            if (sp.plan != c->spill.plan || sp.pcol[0] != c->spill.pcol[0] || sp.pval[1] != c->spill.pval[1] ||
                sp.bucket_cap != c->spill.bucket_cap)
                drop_plan(c);  // a reuse sequence holds the old layout
            c->spill = sp;
            if (guard_bytes()) HIP_TRY(guard_fill(c->gpool_zones, s));  // (nothing of an earlier call is in flight on the pool)
        }
        t->globalMapsNumeric = st.lap();
        return SPECK_OK;
    }

    // ALLOC C: only when nnz changed (Multiply.cu:589-602); publish (Multiply.cu:1116-1121) -- from here C owns c_ro
    int adopt_output()
    {
        const u64 nnz_c = c->h_stats->nnz_c;
        void* c_val = C->data;
        u32* c_col = C->col_ids;
        if (C->nnz != nnz_c || !c_val || !c_col) {
            void* nv = nullptr;
            u32* nc = nullptr;
            hipError_t e1 = guarded_malloc(&nv, std::max<size_t>(nnz_c, 1) * sizeof(T));
            hipError_t e2 = e1 == hipSuccess ? guarded_malloc(reinterpret_cast<void**>(&nc), std::max<size_t>(nnz_c, 1) * 4) : e1;
            if (e1 != hipSuccess || e2 != hipSuccess) {
                if (nv) (void)guarded_free(nv);
                (void)hipGetLastError();
                return SPECK_ERR_OOM;
            }
            if (C->data) (void)guarded_free(C->data);
            if (C->col_ids) (void)guarded_free(C->col_ids);
            if (C->row_offsets && C->row_offsets != c_ro) (void)guarded_free(C->row_offsets);
            c_val = nv;
            c_col = nc;
        } else if (C->row_offsets && C->row_offsets != c_ro) {
            (void)guarded_free(C->row_offsets);
        }
        C->rows = A->rows, C->cols = B->cols, C->nnz = nnz_c;
        C->data = c_val, C->col_ids = c_col, C->row_offsets = c_ro;
        own_ro = false;
        t->allocC = st.lap();
        t->loadBalanceNumeric = 0.f;
        return SPECK_OK;
    }

    // NUMERIC (Multiply.cu:835-1014) + in-kernel sort (Multiply.cu:1028-1043), into the C adopt_output published
    int numeric_two_phase()
    {
        // the staged offsets -> C.row_offsets: by extra workgroups of the numeric light launch when there is one, else by a
        // copy of its own (enqueue_back)
        CallForm staged;
        staged.off_src = sc.offsets, staged.off_dst = C->row_offsets, staged.off_n = m + 1;
        c->prev.g_products = c->h_stats->g_products;
        int rc = timed_numeric([&] { return back(staged, C->col_ids, C->data, num_mask, c->h_stats->num.count); });
        if (rc != SPECK_OK) return rc;
        // The reference may return before its kernels finish when measureCompleteTime is off
        // (Multiply.cu:1082-1085) and relies on blocking streams to order later copies.  The
        // pipeline streams here are non-blocking, so the call always returns with C complete.
        if (c->spin_wait && !c->profile_kernels) {
            launch_done(s, c->d_ticket, c->h_ticket_dev, c->d_stats, c->h_stats_dev);
            rc = wait_ticket(c, s);
            if (rc != SPECK_OK) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(s));
        }
        t->spGEMMNumeric = st.lap();
        return SPECK_OK;
    }

    // remember what this call ran on: the next call on the config is sized from it, an identical one may reuse its placement
    void remember_call(bool walked, Attempt through)
    {
        t->sorting = 0.f;  // sorting is fused into the numeric kernels
        t->cleanup = 0.f;  // nothing to free: the arena persists
        LastCall& prev = c->prev;
        prev.was_walk = walked;
        prev.nf_entries = c->h_stats->nf_entries;
        prev.sym_mask = mask_of(c->h_stats->sym.count, SYM_CLASSES);
        prev.num_mask = num_mask;
        prev.max_row_nnz = c->h_stats->max_row_nnz_c, prev.max_row_ops = c->h_stats->max_row_ops;
        std::memcpy(prev.sym_counts, c->h_stats->sym.count, sizeof(prev.sym_counts));
        std::memcpy(prev.num_counts, c->h_stats->num.count, sizeof(prev.num_counts));
        c->last_key = c->arena_key = make_key<T>(c, A, B, C, s);
        c->last_key_valid = c->arena_key_valid = true;
        c->arena_from_replay = false;
        prev.valid = true, prev.rows_a = A->rows, prev.rows_b = B->rows;
        // ... and where every row went: the scan kernel wrote the config's copy of the offsets as it went
        c->pred_valid = keep_pred;
        prev.eager_stats = *c->h_stats;
        if (through == Attempt::missed || through == Attempt::front_stands) {
            c->last.eager_through = -1;
            if (through == Attempt::missed) c->last.eager_speculated = -1;  // (what the batch was sized from did not hold)
        }
    }

    // the complete time, the times of the kernel events, the reference's table of stage times
    int report_times()
    {
        const int rc = finish_complete();
        if (rc != SPECK_OK) return rc;
        if (c->profile_kernels) {
            HIP_TRY(hipStreamSynchronize(s));
            publish_kernel_times(c, tm, ev_num_end);
            if (t->measureAll) {
                // the reference's eleven stage fields (Timings.h:7-18, filled at Multiply.cu:227-1073) from
                // the kernel events: stages that are fused here report under the field of their role
                t->countProducts = c->last.analysis_ms;                            // readOperations + symbolic binning: ONE kernel
                t->loadBalanceCounting = 0.f;                                     //   since round 5 (stages.hip)
                t->spGEMMCounting = c->last.sym_phase_ms;                          // symbolic launches
                t->loadBalanceNumeric = c->last.scan_ms;                           // scan + numeric binning
                t->spGEMMNumeric = c->last.num_phase_ms;                           // numeric launches ...
                t->sorting = 0.f;                                                  // ... which sort in-kernel
            }
        }
        if (t->measureAll) {
            // same table the reference prints (Multiply.cu:1097-1113)
            const std::pair<const char*, float> rows[] = {
                {"initial mallocs", t->init}, {"count computations", t->countProducts}, {"load-balancer", t->loadBalanceCounting},
                {"GlobalMaps Cnt", t->globalMapsCounting}, {"counting kernel", t->spGEMMCounting}, {"malloc mat C", t->allocC},
                {"num load-balancer", t->loadBalanceNumeric}, {"init GlobalMaps", t->globalMapsNumeric},
                {"numeric kernel", t->spGEMMNumeric}, {"Sorting kernel", t->sorting}, {"cleanup", t->cleanup}};
            for (const auto& r : rows) std::printf("spECK %19s = %f ms\n", r.first, r.second);
            std::printf("--------------------------------------------------------------\n");
        }
        return SPECK_OK;
    }
};

// The dispatcher: argument checks, the product of an empty input, arena and zones, then the kinds of call in their order
//  -- each attempt completes the call, does not apply, or misses and hands over to the next
template <typename T>
int multiply_impl(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, speck_dcsr* C,
                  speck_timings* t)
{
    if (!c || !C) return SPECK_ERR_INVALID;
    int rc = check_inputs(A, B);
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    speck_timings local_t{};
    if (!t) t = &local_t;
    c->last = speck_stats{};
    // reference: source/GPU/Multiply.cu:67-70
    if (A->nnz == 0 || B->nnz == 0) {
        C->nnz = 0;
        return SPECK_OK;
    }
    hipStream_t s = main_stream(c);
    rc = check_view_below_the_top(A, s);
    if (rc != SPECK_OK) return rc;
    if (t->measureCompleteTime) HIP_TRY(hipEventRecord(c->completeStart, s));
    Call<T> k(c, A, B, C, t, s);
    struct RestoreFlag {
        int& flag;
        int value;
        ~RestoreFlag() { flag = value; }
    } restore_profile{c->profile_kernels, c->profile_kernels};
    if (t->measureAll) c->profile_kernels = 1;  // per-stage times come from per-launch events

    rc = ensure_arena(c, scratch_bytes(k.m, A->nnz));
    if (rc != SPECK_OK) return rc;
    std::vector<GuardZone> carved;
    k.sc = carve(c, k.m, A->nnz, guard_bytes() ? &carved : nullptr);
    if (guard_bytes() && (c->zones_arena != c->arena || c->zones_m != k.m || c->zones_nnz != A->nnz || c->zones_gap != guard_bytes())) {
        // (another layout of the arena than the one whose zones were filled last: canaries between ITS regions)
        HIP_TRY(guard_fill(carved, s));
        c->arena_zones = carved;
        c->zones_arena = c->arena, c->zones_m = k.m, c->zones_nnz = A->nnz, c->zones_gap = guard_bytes();
    }
    c->snap_pending = false;
    if (c->verify_inputs && c->overlap_analysis && c->reuse) ensure_snap(c, A->nnz, B->rows);
    VerifierGuard verifier_guard{c};

    Attempt how = Attempt::not_tried, walk = Attempt::not_tried, through = Attempt::not_tried;
    rc = k.try_replay(how);
    if (rc != SPECK_OK || how == Attempt::done) return rc;
    rc = k.begin_complete();
    if (rc != SPECK_OK) return rc;
    rc = k.try_walk_hash(how);
    if (rc != SPECK_OK || how == Attempt::done) return rc;
    rc = k.try_one_walk(walk);
    if (rc != SPECK_OK) return rc;
    const bool walked = walk == Attempt::done;
    if (!walked) rc = k.try_through(through);
    if (rc != SPECK_OK) return rc;
    if (!walked && through != Attempt::done) {
        // the two-phase call: a front (the through call's if it stands, else a speculated batch, else the plain one with
        // its read-backs), then on the host nnz(C), the spill pool and C, then the numeric launches
        bool front_held = through == Attempt::front_stands, empty = false;
        if (front_held) c->last.eager_speculated = 1;
        if (through == Attempt::not_tried) rc = k.front_speculated(&front_held);
        if (rc == SPECK_OK && !front_held) rc = k.front_two_phase();
        if (rc == SPECK_OK) rc = k.settle_front(&empty);
        if (rc != SPECK_OK || empty) return rc;
        rc = k.size_spill_pool();
        if (rc == SPECK_OK) rc = k.adopt_output();
        if (rc == SPECK_OK) rc = k.numeric_two_phase();
        if (rc != SPECK_OK) return rc;
    }
    k.remember_call(walked, through);
    return k.report_times();
}

}  // namespace

namespace speck {
SortScratch* sort_scratch(speck_config* c) { return &c->sort; }
hipStream_t call_stream(speck_config* c) { return main_stream(c); }
MaskedScratch* masked_scratch(speck_config* c) { return &c->masked; }

SelectScratch* select_scratch(speck_config* c) { return &c->select; }
AddScratch* add_scratch(speck_config* c) { return &c->add; }
TileScratch* reduce_scratch(speck_config* c) { return &c->reduce; }
ScaleScratch* scale_scratch(speck_config* c) { return &c->scale; }
TileScratch* spmv_scratch(speck_config* c) { return &c->spmv; }
TileScratch* spmm_scratch(speck_config* c) { return &c->spmm; }
ScaleScratch* sddmm_scratch(speck_config* c) { return &c->sddmm; }
TileScratch* softmax_scratch(speck_config* c) { return &c->softmax; }
TileScratch* spmm_t_scratch(speck_config* c) { return &c->spmm_t; }
TileScratch* spmv_sr_scratch(speck_config* c) { return &c->spmv_sr; }
TileScratch* spmm_sr_scratch(speck_config* c) { return &c->spmm_sr; }
CooScratch* coo_scratch(speck_config* c) { return &c->coo; }
ExtractScratch* extract_scratch(speck_config* c) { return &c->extract; }
TopKScratch* topk_scratch(speck_config* c) { return &c->topk; }
SampleScratch* sample_scratch(speck_config* c) { return &c->sample; }
BmatScratch* bmat_scratch(speck_config* c) { return &c->bmat; }
}  // namespace speck

extern "C" {

int speck_config_create(int device, speck_config** out)
{
    if (!out) return SPECK_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) {
        (void)hipGetLastError();
        return SPECK_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    auto* c = new speck_config();
    c->device = device;
    c->sm = prop.multiProcessorCount;
    c->max_static_lds = (int)prop.sharedMemPerBlock;
    c->max_dynamic_lds = (int)std::max(prop.sharedMemPerBlockOptin, prop.sharedMemPerBlock);
    for (int i = 0; i < 6; ++i) {
        hipStream_t s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        c->streams.push_back(s);
    }
    HIP_TRY(hipEventCreate(&c->completeStart));
    HIP_TRY(hipEventCreate(&c->completeEnd));
    HIP_TRY(hipEventCreate(&c->individualStart));
    HIP_TRY(hipEventCreate(&c->individualEnd));
    for (int i = 0; i < kMaxClasses; ++i) {
        hipStream_t s;
        hipEvent_t e;
        // (a HIGH-priority stream for the NUM_G chain -- seven short kernels that queue for LDS behind the long rows of
        //  the other launches -- was tried in round 4: the webbase stand-in lost 5 %, and the mere existence of such a
        //  stream cost the scircuit stand-in, which never uses it, 55 %: 0.088 -> 0.138 ms.  Not done.)
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->aux.push_back(s);
        c->aux_done.push_back(e);
    }
    HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->vgate, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->vdone, hipEventDisableTiming));
    {
        // the verifier yields to the sequence it runs beside: lowest stream priority (the sequence's light launches
        // lost 5-8 % to it at equal priority)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        HIP_TRY(hipStreamCreateWithPriority(&c->vstream, hipStreamNonBlocking, least));
    }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_verify), 128, hipHostMallocMapped));
    std::memset(c->h_verify, 0, 128);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_vticket), sizeof(u32)));
    HIP_TRY(hipMemset(c->d_vticket, 0, sizeof(u32)));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_verify_dev), c->h_verify, 0));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_stats), sizeof(DeviceStats)));
    HIP_TRY(hipMemset(c->d_stats, 0, sizeof(DeviceStats)));
    // the look-back chain of the analysis / scan kernels: tags and epoch start from zero, once (chain.hpp)
    HIP_TRY(hipMalloc(&c->chain_buf, 2 * kChainBytes));
    HIP_TRY(hipMemset(c->chain_buf, 0, 2 * kChainBytes));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_bytes), 2 * kMaxClasses * sizeof(u64)));
    HIP_TRY(hipMemset(c->d_bytes, 0, 2 * kMaxClasses * sizeof(u64)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_stats), sizeof(DeviceStats), hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_stats_dev), c->h_stats, 0));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_ticket), sizeof(u32)));
    HIP_TRY(hipMemset(c->d_ticket, 0, sizeof(u32)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_ticket), 64, hipHostMallocMapped));
    *c->h_ticket = 0;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_ticket_dev), c->h_ticket, 0));
    c->cp.sym_bitmap_ratio = 32;
    c->cp.num_dense_ratio = 16;
    c->cp.num_global_passes = 4;  // heavy rows: dense windows up to 64 Ki columns, else global spill
    c->cp.nf_min_ops = 512;   // numeric-first for narrow rows with at least this many products (0 = off; 256 costs the
                              // scircuit stand-in 5 %, 1024 leaves the boundary rows of the cant one a launch of their own)
    c->cp.gh_per_window = 8192;  // global key set for rows with fewer products per 1 Mi-column bitmap window (0 = off)
    c->cp.esc16 = 1;       // rows of <= 64 products from <= 16 entries: 16 lanes per row, in registers (esc.hpp)
    c->cp.esc32 = 1;       // rows of <= 128 products from <= 32 entries: 32 lanes per row, in registers (esc_wide.hpp)
    c->cp.esc64 = 1;       // rows of <= 256 products from <= 64 entries: a wave per row, in registers
    c->cp.num_g8 = 1;      // rows of <= 32 products from <= 8 entries: 8 lanes per row, in registers
    c->cp.sym_g8 = 1;      // rows of <= 25 products: 8 lanes per row
    c->cp.sym_w128 = 1;    // rows of 52..102 products: 16 lanes per row
    c->cp.num_w256 = 1;    // rows of 86..170 entries: 32 lanes per row
    c->cp.want_bytes = 0;
    c->cp.slice_ops = 0;   // option slice_rows: NUM_B8K rows in column slices of the 2 Ki table (num_sliced_body) -- measured
                           //   and lost on the webbase stand-in (1.16 -> 1.23 ms), off
    *out = c;
    return SPECK_OK;
}

int speck_config_destroy(speck_config* c)
{
    if (!c) return SPECK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto s : c->streams) (void)hipStreamDestroy(s);
    (void)hipEventDestroy(c->completeStart);
    (void)hipEventDestroy(c->completeEnd);
    (void)hipEventDestroy(c->individualStart);
    (void)hipEventDestroy(c->individualEnd);
    for (auto e : c->kev) (void)hipEventDestroy(e);
    for (auto s : c->aux) (void)hipStreamDestroy(s);
    for (auto e : c->aux_done) (void)hipEventDestroy(e);
    if (c->fork) (void)hipEventDestroy(c->fork);
    if (c->vgate) (void)hipEventDestroy(c->vgate);
    if (c->vdone) (void)hipEventDestroy(c->vdone);
    if (c->vstream) (void)hipStreamDestroy(c->vstream);
    if (c->h_verify) (void)hipHostFree(c->h_verify);
    if (c->d_vticket) (void)hipFree(c->d_vticket);
    if (c->arena) (void)guarded_free(c->arena);
    if (c->snap) (void)guarded_free(c->snap);
    if (c->gpool) (void)guarded_free(c->gpool);
    if (c->nfpool) (void)guarded_free(c->nfpool);
    c->sort.release();
    c->masked.release();
    c->select.release();
    c->add.release();
    c->reduce.release();
    c->scale.release();
    c->spmv.release();
    c->spmm.release();
    c->sddmm.release();
    c->softmax.release();
    c->spmm_t.release();
    c->spmv_sr.release();
    c->spmm_sr.release();
    c->coo.release();
    c->extract.release();
    c->topk.release();
    c->sample.release();
    c->bmat.release();
    if (c->pred.off) (void)guarded_free(c->pred.off);
    if (c->gpred.off) (void)guarded_free(c->gpred.off);
    if (c->d_stats) (void)hipFree(c->d_stats);
    if (c->chain_buf) (void)hipFree(c->chain_buf);
    if (c->chain3_buf) (void)guarded_free(c->chain3_buf);
    if (c->d_bytes) (void)hipFree(c->d_bytes);
    if (c->h_stats) (void)hipHostFree(c->h_stats);
    if (c->h_ticket) (void)hipHostFree(c->h_ticket);
    if (c->d_ticket) (void)hipFree(c->d_ticket);
    delete c;
    return SPECK_OK;
}

int speck_config_info(const speck_config* c, int* sm, int* max_static_lds, int* max_dynamic_lds)
{
    if (!c) return SPECK_ERR_INVALID;
    if (sm) *sm = c->sm;
    if (max_static_lds) *max_static_lds = c->max_static_lds;
    if (max_dynamic_lds) *max_dynamic_lds = c->max_dynamic_lds;
    return SPECK_OK;
}

int speck_config_handles(const speck_config* c, void* streams6[6], void* events4[4])
{
    if (!c) return SPECK_ERR_INVALID;
    if (streams6)
        for (int i = 0; i < 6; ++i) streams6[i] = c->streams[i];
    if (events4) {
        events4[0] = c->completeStart;
        events4[1] = c->completeEnd;
        events4[2] = c->individualStart;
        events4[3] = c->individualEnd;
    }
    return SPECK_OK;
}

int speck_config_set_stream(speck_config* c, void* hip_stream)
{
    if (!c) return SPECK_ERR_INVALID;
    c->user_stream = static_cast<hipStream_t>(hip_stream);
    c->use_user_stream = hip_stream != nullptr;
    drop_plan(c);  // (a sequence is tied to the stream it was made for, and to HOW it is replayed there)
    return SPECK_OK;
}

int speck_config_set_option(speck_config* c, const char* name, int64_t value)
{
    if (!c || !name) return SPECK_ERR_INVALID;
    const std::string n(name);
    // every option a test or a script sets; anything that changes how rows are classified or what a reuse sequence
    // may take for granted also forgets the sequence (and the complete call it was planned from)
    auto forget = [&](bool also_last_call) {
        drop_plan(c);
        if (also_last_call) c->last_key_valid = false;
    };
    if (n == "sym_bitmap_ratio") c->cp.sym_bitmap_ratio = (u32)value;
    else if (n == "num_dense_ratio") c->cp.num_dense_ratio = (u32)value;
    else if (n == "num_global_passes") c->cp.num_global_passes = (u32)value;
    else if (n == "gh_per_window") c->cp.gh_per_window = (u32)value, forget(true);
    else if (n == "nf_min_ops") c->cp.nf_min_ops = (u32)value, forget(true);
    else if (n == "nf_pool_max_mb") c->nf_pool_max_bytes = size_t(value) << 20;
    else if (n == "analysis_wide_rows") set_analysis_wide_rows((u32)value), forget(true);
    else if (n == "eager_speculate") c->eager_speculate = value != 0;
    else if (n == "eager_through") c->eager_through = value != 0;
    else if (n == "one_walk") c->one_walk = (int)value;
    else if (n == "one_walk_hash") c->one_walk_hash = (int)value;
    else if (n == "walk_hash_debug") c->walk_hash_debug = (u32)value;
    else if (n == "chain_fault") c->chain_fault = (u32)value;
    else if (n == "guard_bytes") {
        // debug (guards.hpp): canary zones of `value` bytes around / inside everything allocated FROM NOW ON -- the
        // config's own buffers are dropped so that they come back with zones
        (void)hipDeviceSynchronize();
        set_guard_bytes((size_t)value);
        forget(true);
        c->arena_bytes = 0, c->arena_key_valid = false, c->zones_arena = nullptr, c->arena_zones.clear();
        if (c->nfpool) (void)guarded_free(c->nfpool);
        c->nfpool = nullptr, c->nfpool_bytes = 0, c->nf_cap_entries = 0, c->nfpool_zones.clear();
        if (c->gpool) (void)guarded_free(c->gpool);
        c->gpool = nullptr, c->gpool_bytes = 0, c->gpool_zones.clear(), c->spill = SpillBuffers{};
        c->prev.valid = false;
        c->sort.release();
        c->masked.release();
        c->select.release();
        c->add.release();
        c->reduce.release();
        c->scale.release();
        c->spmv.release();
        c->spmm.release();
        c->sddmm.release();
        c->softmax.release();
        c->spmm_t.release();
        c->spmv_sr.release();
        c->spmm_sr.release();
        c->coo.release();
        c->extract.release();
        c->topk.release();
        c->sample.release();
        c->bmat.release();
    }
    else if (n == "sort_reg_max") c->sort.reg_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_SORT_REG_MAX);
    else if (n == "sort_lds_max") c->sort.lds_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_SORT_LDS_MAX);
    else if (n == "topk_group_max") c->topk.group_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_TOPK_GROUP_MAX);
    else if (n == "topk_lds_max") c->topk.lds_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_TOPK_LDS_MAX);
    else if (n == "sample_group_max") c->sample.group_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_SAMPLE_GROUP_MAX);
    else if (n == "sample_lds_max") c->sample.lds_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_SAMPLE_LDS_MAX);
    else if (n == "mask_group_max") c->masked.group_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_MASK_GROUP_MAX);
    else if (n == "mask_lds_max") c->masked.lds_max = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), SPECK_MASK_LDS_MAX);
    else if (n == "walk_debug") set_walk_debug((u32)value & 0xFFFFu, (u32)(value >> 16));  // (tile rows | flags << 16)
    else if (n == "verify_inputs") c->verify_inputs = value != 0, c->snap_for_arena = false, forget(false);
    else if (n == "num_verify") c->num_verify = (int)value, forget(false);
    else if (n == "skip_scan") c->skip_scan = value != 0, forget(false);
    else if (n == "overlap_analysis") c->overlap_analysis = value != 0, forget(false);
    else if (n == "esc_fused") c->esc_fused = value != 0, forget(true);
    else if (n == "nf_direct") c->nf_direct = value != 0, forget(false);
    else if (n == "sym_w128") c->cp.sym_w128 = value != 0, forget(true);
    else if (n == "sym_g8") c->cp.sym_g8 = value != 0, forget(true);
    else if (n == "esc16") c->cp.esc16 = value != 0, forget(true);
    else if (n == "slice_rows") c->cp.slice_ops = value ? kSliceMaxOps : 0u, forget(true);
    else if (n == "esc32") c->cp.esc32 = value != 0, forget(true);
    else if (n == "esc64") c->cp.esc64 = value != 0, forget(true);
    else if (n == "num_g8") c->cp.num_g8 = value != 0, forget(true);
    else if (n == "num_w256") c->cp.num_w256 = value != 0, forget(true);
    else if (n == "collect_bytes") c->cp.want_bytes = value != 0;        // per-class byte model
    else if (n == "concurrent_classes") c->concurrent_classes = value != 0;
    else if (n == "validate_inputs") c->validate_inputs = value != 0;
    else if (n == "validate_after_nnz") c->validate_after_nnz = (u64)value;
    else if (n == "spin_wait") c->spin_wait = value != 0, forget(false);
    else if (n == "fork_min_us") c->fork_min_us = (float)value, forget(false);
    else if (n == "max_side_streams") c->max_side_streams = (u32)value, forget(false);
    else if (n == "reuse" || n == "use_graph") {  // ("use_graph": the name of rounds 2-4, kept)
        // (a complete call leaves its row offsets behind only for a config that may reuse them: the call that follows
        //  the switch is a complete one)
        if (c->reuse != (value != 0)) forget(true);
        c->reuse = value != 0;
    }
    else if (n == "grid_rounds_block") set_grid_rounds((u32)value, 0), forget(false);
    else if (n == "grid_rounds_sub") set_grid_rounds(0, (u32)value), forget(false);
    else if (n == "esc_walk_rows") set_esc_walk((u32)std::max<int64_t>(value, 1), -1), forget(false);
    else if (n == "esc_walk_resident") set_esc_walk(0, std::max<int64_t>(value, 0)), forget(false);  // (debug: 0 = the runtime's figure)
    else if (n == "spill_big_grid") set_spill_big_grid((u32)value), forget(false);
    else if (n == "scan_small_items") set_scan_small_items((int)value), forget(true);
    else if (n == "b8k_full_first") set_b8k_full_first((u32)value), forget(false);
    else if (n == "xcd_aware") c->xcd_aware = (u32)value, forget(false);
    else return SPECK_ERR_INVALID;
    return SPECK_OK;
}

int speck_config_profile_kernels(speck_config* c, int enable)
{
    if (!c) return SPECK_ERR_INVALID;
    c->profile_kernels = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return SPECK_OK;
}

int speck_last_stats(const speck_config* c, speck_stats* out)
{
    if (!c || !out) return SPECK_ERR_INVALID;
    *out = c->last;
    out->numeric_reruns = c->replay_misses;
    out->graph_replays = c->replays;
    out->graph_captures = c->plans_made;
    out->pool_fallbacks = c->pool_fallbacks;
    out->scratch_pool_bytes = c->nfpool_bytes;
    out->walk_misses = c->walk_misses;
    return SPECK_OK;
}

// debug option guard_bytes: every canary zone of the config's buffers and of C after the call (guards.hpp)
static int check_guards(speck_config* c, const speck_dcsr* C, int rc)
{
    if (!guard_bytes() || !c) return rc;
    std::vector<GuardZone> inner = c->arena_zones;
    inner.insert(inner.end(), c->gpool_zones.begin(), c->gpool_zones.end());
    inner.insert(inner.end(), c->nfpool_zones.begin(), c->nfpool_zones.end());
    const void* whole[] = {c->arena, c->snap, c->pred.off, c->gpred.off, c->nfpool, c->gpool,
                           C ? C->data : nullptr, C ? C->col_ids : nullptr, C ? C->row_offsets : nullptr};
    static const char* names[] = {"arena", "input snapshot", "row-offset copy", "row-offset copy (sequence)", "scratch pool",
                                  "spill pool", "C.data", "C.col_ids", "C.row_offsets"};
    return guard_check_buffers(whole, names, 9, main_stream(c), nullptr, rc, std::move(inner));
}

int speck_multiply_f64(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, speck_dcsr* C,
                       speck_timings* t)
{
    return check_guards(c, C, multiply_impl<double>(c, A, B, C, t));
}

int speck_multiply_f32(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, speck_dcsr* C,
                       speck_timings* t)
{
    return check_guards(c, C, multiply_impl<float>(c, A, B, C, t));
}

int speck_analysis(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, uint32_t* d_row_ops,
                   uint32_t* d_row_max_ops, uint32_t* d_row_col_min, uint32_t* d_row_col_max,
                   uint64_t* h_sum_products, uint32_t* h_max_row_ops)
{
    if (!c) return SPECK_ERR_INVALID;
    int rc = check_inputs(A, B);
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = main_stream(c);
    rc = check_view_below_the_top(A, s);
    if (rc != SPECK_OK) return rc;
    c->arena_key_valid = false;  // (... and writes the arena)
    const u32 m = (u32)A->rows;
    if (m == 0 || A->nnz == 0 || B->nnz == 0) {
        if (h_sum_products) *h_sum_products = 0;
        if (h_max_row_ops) *h_max_row_ops = 0;
        if (m) {
            if (d_row_ops) HIP_TRY(hipMemsetAsync(d_row_ops, 0, size_t(m) * 4, s));
            if (d_row_max_ops) HIP_TRY(hipMemsetAsync(d_row_max_ops, 0, size_t(m) * 4, s));
            if (d_row_col_min) HIP_TRY(hipMemsetAsync(d_row_col_min, 0xFF, size_t(m) * 4, s));
            if (d_row_col_max) HIP_TRY(hipMemsetAsync(d_row_col_max, 0, size_t(m) * 4, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return SPECK_OK;
    }
    rc = ensure_arena(c, scratch_bytes(m, A->nnz));
    if (rc != SPECK_OK) return rc;
    Scratch sc = carve(c, m, A->nnz);  // (the row arrays come from the caller)
    ClassifyParams cp = c->cp;
    cp.sym_allowed = cp.num_allowed = 0xFFFFFFFFu;
    Chain chain;
    rc = next_chain(c, s, &chain);
    if (rc != SPECK_OK) return rc;
    launch_analysis(s, A->row_offsets, A->col_ids, B->row_offsets, B->col_ids, m, A->nnz, d_row_ops, d_row_max_ops,
                    d_row_col_min, d_row_col_max, nullptr, nullptr, sc.sym_recs, c->d_stats, cp, nullptr, chain,
                    nullptr, ~0ull, (u32)B->rows, nullptr, nullptr, nullptr, B->nnz);
    LAUNCHES_OK();
    rc = read_stats(c, s);
    if (rc != SPECK_OK) return rc;
    if (c->h_stats->a_invalid) return SPECK_ERR_INVALID;
    if (h_sum_products) *h_sum_products = c->h_stats->sum_products;
    if (h_max_row_ops) *h_max_row_ops = c->h_stats->max_row_ops;
    return SPECK_OK;
}

int speck_symbolic(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, uint32_t* d_row_offsets,
                   uint64_t* h_nnz_c)
{
    if (!c || !d_row_offsets) return SPECK_ERR_INVALID;
    int rc = check_inputs(A, B);
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = main_stream(c);
    rc = check_view_below_the_top(A, s);
    if (rc != SPECK_OK) return rc;
    c->arena_key_valid = false;  // (... and writes the arena)
    const u32 m = (u32)A->rows;
    if (A->nnz == 0 || B->nnz == 0) {
        HIP_TRY(hipMemsetAsync(d_row_offsets, 0, (size_t(m) + 1) * 4, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_nnz_c) *h_nnz_c = 0;
        return SPECK_OK;
    }
    rc = ensure_arena(c, scratch_bytes(m, A->nnz));
    if (rc != SPECK_OK) return rc;
    Scratch sc = carve(c, m, A->nnz);
    const u32 nf_was = c->cp.nf_min_ops, gh_was = c->cp.gh_per_window;
    c->cp.nf_min_ops = 0;  // structure only: no values here, every row through a symbolic kernel
    c->cp.gh_per_window = 0;  // ... one that needs no scratch pool
    CallForm f;  // (no form of a multiply: only the window the symbolic phase's numeric-first launch is sized with)
    f.nf_wcols = c->nf_wcols;
    FrontArgs fa;
    fa.classify_numeric = false;
    rc = enqueue_front(c, s, A, B, sc, 8, f, fa, nullptr);
    c->cp.nf_min_ops = nf_was;
    c->cp.gh_per_window = gh_was;
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_row_offsets, sc.offsets, (size_t(m) + 1) * 4, hipMemcpyDeviceToDevice, s));
    rc = read_stats(c, s);
    if (rc != SPECK_OK) return rc;
    c->last_key_valid = false;
    if (c->h_stats->nnz_overflow) return SPECK_ERR_NNZ_OVERFLOW;
    if (h_nnz_c) *h_nnz_c = c->h_stats->nnz_c;
    return SPECK_OK;
}

int speck_partition_rows(speck_config* c, const speck_dcsr* A, const speck_dcsr* B, int parts,
                         uint64_t* h_bounds)
{
    if (!c || !h_bounds || parts <= 0) return SPECK_ERR_INVALID;
    int rc = check_inputs(A, B);
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = check_view_below_the_top(A, main_stream(c));
    if (rc != SPECK_OK) return rc;
    const u32 m = (u32)A->rows;
    rc = ensure_arena(c, scratch_bytes(m, A->nnz));
    if (rc != SPECK_OK) return rc;
    Scratch sc = carve(c, m, A->nnz);
    u64 P = 0;
    rc = speck_analysis(c, A, B, sc.row_ops, nullptr, nullptr, nullptr, &P, nullptr);
    if (rc != SPECK_OK) return rc;
    std::vector<u32> ops(m);
    if (m) HIP_TRY(hipMemcpy(ops.data(), sc.row_ops, size_t(m) * 4, hipMemcpyDeviceToHost));
    // cost per row: products plus a per-row constant so that empty rows still spread
    h_bounds[0] = 0;
    u64 total = P + m;
    u64 run = 0;
    int next = 1;
    for (u32 i = 0; i < m && next < parts; ++i) {
        run += u64(ops[i]) + 1;
        while (next < parts && run * parts >= total * next) h_bounds[next++] = i + 1;
    }
    while (next <= parts) h_bounds[next++] = m;
    return SPECK_OK;
}

const char* speck_status_string(int status)
{
    switch (status) {
        case SPECK_OK: return "ok";
        case SPECK_ERR_INVALID: return "invalid argument";
        case SPECK_ERR_DIM_LIMIT: return "matrix dimension above the 2^27 limit";
        case SPECK_ERR_HIP: return "HIP runtime error";
        case SPECK_ERR_OOM: return "out of device memory";
        case SPECK_ERR_NNZ_OVERFLOW: return "nnz(C) exceeds 2^32-1 (u32 row_offsets)";
        case SPECK_ERR_NO_DEVICE: return "no such HIP device";
        case SPECK_ERR_IO: return "I/O error";
        case SPECK_ERR_UNSORTED: return "a row of B is not strictly ascending (or holds a column >= cols)";
        case SPECK_ERR_COMM: return "multi-GPU exchange failed (RCCL / shared-memory transport)";
    }
    return "unknown";
}

const char* speck_version(void) { return "speck_amd 0.4 (gfx950)"; }

}  // extern "C"
