// KeyFrameDatabase (src/KeyFrameDatabase.cc:39-98 container, :601-669 and :738-792 the place-recognition query up to the scores;
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68 the L1 score) on BowVectors that stay on the device.
//
// The reference keeps an inverted file (word -> std::list of KeyFrames).  A query walks the lists of its words in ascending word id
// and, per KeyFrame met, counts the encounters (= the size of the word intersection); the KeyFrames come out in first-encounter
// order, i.e. ordered by (smallest common word, position in that word's list = add order).  Those above a share of the largest
// count are then scored by a merge walk over the two sorted vectors that adds, in double and in ascending word order,
// fabs(vi - wi) - fabs(vi) - fabs(wi) per common word.
//
// Here the database is the forward file: per entry one ascending int32 word row and one double value row in two device arrays
// (rows reused first fit, as the KeyFrame store of bow_match.hip does).  One kernel pass over the rows gives, for every live entry,
// the common-word count, the smallest common word and the score of the reference's double additions in the reference's order; the
// host orders the sharing entries by (smallest common word, add sequence) and applies the threshold arithmetic.  A wavefront owns
// an entry: its lanes take 64 consecutive stored words (coalesced), each binary-searches the query's word table (in LDS, sized to
// the query; in global memory when the query does not fit), the hits are a ballot, the count a population count, and the running
// double is advanced hit by hit in lane order (= ascending word order) by a broadcast and one f64 add.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "lds_limit.h"
#include "store_arena.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;

namespace {

struct KfdbRec {   // one entry id
    long long begin;   // first element of its rows in the word / value arrays
    int n;             // words
    int alive;
};
struct KfdbOut {   // per entry id, written for every id below the bound
    double score;   // ScoringObject.cpp:65: -score / 2.0 (a double; the reference narrows it to float at KeyFrameDatabase.cc:663 / :788)
    int common;     // words the entry shares with the query (0: not sharing, or not alive)
    int first;      // the smallest of them (-1 when common == 0)
};
static_assert(sizeof(KfdbRec) == 16 && sizeof(KfdbOut) == 16, "staging layout");

constexpr int kWaves = 4;   // wavefronts (= entries in flight) per workgroup

// QLDS: the query's table is copied to dynamic LDS ([nq doubles | nq ints]) once per workgroup; otherwise it is searched where it is.
template <bool QLDS>
__global__ __launch_bounds__(kWaves * 64) void kfdb_query_kernel(const int* __restrict__ q_word, const double* __restrict__ q_value, int nq,
                                                                  const KfdbRec* __restrict__ rec, int id_bound,
                                                                  const int* __restrict__ words, const double* __restrict__ values,
                                                                  KfdbOut* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double kfdb_lds[];   // no static LDS in this kernel: the base stays aligned
    const int* tw = q_word;
    const double* tv = q_value;
    if (QLDS) {
        double* sv = kfdb_lds;
        int* sw = reinterpret_cast<int*>(kfdb_lds + nq);
        for (int i = threadIdx.x; i < nq; i += kWaves * 64) { sv[i] = q_value[i]; sw[i] = q_word[i]; }
        __syncthreads();
        tw = sw;
        tv = sv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long id = (long long)blockIdx.x * kWaves + wave; id < id_bound; id += (long long)gridDim.x * kWaves) {
        const KfdbRec r = rec[id];
        int common = 0, first = -1;
        double sum = 0;   // ScoringObject.cpp:32
        if (r.alive) {
            for (int base = 0; base < r.n; base += 64) {
                const int k = base + lane;
                bool hit = false;
                int w = 0;
                double term = 0;
                if (k < r.n) {
                    w = words[r.begin + k];
                    int lo = 0, hi = nq;   // first table entry >= w
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (tw[mid] < w) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < nq && tw[lo] == w) {
                        hit = true;
                        const double vi = tv[lo], wi = values[r.begin + k];   // v1 = the query, v2 = the stored vector (:663, :788)
                        term = fabs(vi - wi) - fabs(vi) - fabs(wi);           // ScoringObject.cpp:41
                    }
                }
                unsigned long long m = __ballot(hit);
                if (m) {
                    if (first < 0) first = __shfl(w, __ffsll((long long)m) - 1);
                    common += __popcll(m);
                    const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
                    while (m) {   // one add per common word, ascending: the order is part of the double
                        const int l = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        sum += __hiloint2double(__builtin_amdgcn_readlane(t_hi, l), __builtin_amdgcn_readlane(t_lo, l));
                    }
                }
            }
        }
        if (lane == 0) {
            KfdbOut o;
            o.score = -sum / 2.0;   // ScoringObject.cpp:65
            o.common = common;
            o.first = first;
            out[id] = o;
        }
    }
}

int hip_fail(ThreadScratch& scr, const char* what, hipError_t e) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    scr.release();
    return MSORB_E_HIP;
}

// words strictly ascending inside [0, n_words)
bool bow_vector_ok(const int* word, int n, int n_words) {
    for (int i = 0; i < n; i++)
        if (word[i] < 0 || word[i] >= n_words || (i && word[i] <= word[i - 1])) return false;
    return true;
}

}  // namespace

struct msorb_kf_database {
    int device = 0, n_words = 0;
    mutable std::shared_mutex mu;   // queries hold it shared (the arrays must not move under a running kernel), add / erase / clear exclusive
    struct Entry {
        bool alive = false;
        size_t row0 = 0;
        int n = 0;
        unsigned long long seq = 0;   // add sequence number: the entry's position in every list of the reference's inverted file
    };
    std::vector<Entry> e;
    std::vector<int> dead_ids;   // ids of erased entries, handed out again by the next add
    int n_alive = 0;
    unsigned long long next_seq = 0;
    msorb::RangeAlloc rows_a;
    size_t rows_cap = 0, rec_cap = 0;
    int* d_word = nullptr;
    double* d_value = nullptr;
    KfdbRec* d_rec = nullptr;
};

extern "C" int msorb_kf_database_create(int device, int n_words, msorb_kf_database** out) {
    if (!out) return MSORB_E_INVALID;
    *out = nullptr;
    if (n_words < 1) { set_last_error("kf_database_create: n_words < 1"); return MSORB_E_INVALID; }
    if (int rc = msorb::require_device(device)) return rc;
    msorb_kf_database* db = new msorb_kf_database();
    db->device = device;
    db->n_words = n_words;
    *out = db;
    return MSORB_OK;
}

extern "C" void msorb_kf_database_destroy(msorb_kf_database* db) {
    if (!db) return;
    if (hipSetDevice(db->device) == hipSuccess) {
        if (db->d_word) (void)hipFree(db->d_word);
        if (db->d_value) (void)hipFree(db->d_value);
        if (db->d_rec) (void)hipFree(db->d_rec);
    }
    delete db;
}

extern "C" int msorb_kf_database_add(msorb_kf_database* db, const int* word, const double* value, int n, int* entry_id) {
    if (!db || !entry_id || n < 0 || (n > 0 && (!word || !value))) return MSORB_E_INVALID;
    *entry_id = -1;
    if (!bow_vector_ok(word, n, db->n_words)) {
        set_last_error("kf_database_add: word ids must be strictly ascending and below n_words");
        return MSORB_E_INVALID;
    }
    std::unique_lock<std::shared_mutex> lk(db->mu);
    if (hipSetDevice(db->device) != hipSuccess) return MSORB_E_HIP;
    const bool reuse = !db->dead_ids.empty();
    const int id = reuse ? db->dead_ids.back() : (int)db->e.size();
    const size_t used_rows = db->rows_a.end, used_rec = db->e.size();
    const size_t row0 = db->rows_a.take((size_t)n);
    size_t cap_w = db->rows_cap, cap_v = db->rows_cap;
    hipError_t e = msorb::grow(db->d_word, used_rows, cap_w, db->rows_a.end, 1);
    if (e == hipSuccess) e = msorb::grow(db->d_value, used_rows, cap_v, db->rows_a.end, 1);
    if (e == hipSuccess) db->rows_cap = std::min(cap_w, cap_v);
    if (e == hipSuccess) e = msorb::grow(db->d_rec, used_rec, db->rec_cap, (size_t)id + 1, 1);
    if (e == hipSuccess && n) e = hipMemcpy(db->d_word + row0, word, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(db->d_value + row0, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    const KfdbRec r{(long long)row0, n, 1};
    if (e == hipSuccess) e = hipMemcpy(db->d_rec + id, &r, sizeof r, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        db->rows_a.give(row0, (size_t)n);
        set_last_error(std::string("kf_database_add: ") + hipGetErrorString(e));
        return MSORB_E_HIP;
    }
    msorb_kf_database::Entry E;
    E.alive = true; E.row0 = row0; E.n = n; E.seq = db->next_seq++;
    if (reuse) { db->dead_ids.pop_back(); db->e[id] = E; }
    else db->e.push_back(E);
    db->n_alive++;
    *entry_id = id;
    return MSORB_OK;
}

extern "C" int msorb_kf_database_erase(msorb_kf_database* db, int entry_id) {
    if (!db) return MSORB_E_INVALID;
    std::unique_lock<std::shared_mutex> lk(db->mu);
    if (entry_id < 0 || entry_id >= (int)db->e.size() || !db->e[entry_id].alive) {
        set_last_error("kf_database_erase: unknown entry id");
        return MSORB_E_INVALID;
    }
    if (hipSetDevice(db->device) != hipSuccess) return MSORB_E_HIP;
    const KfdbRec r{0, 0, 0};
    HIPCHK(hipMemcpy(db->d_rec + entry_id, &r, sizeof r, hipMemcpyHostToDevice));
    msorb_kf_database::Entry& E = db->e[entry_id];
    E.alive = false;
    db->rows_a.give(E.row0, (size_t)E.n);   // the rows and the id are free for the next add (no kernel is running: the lock is exclusive)
    E.n = 0;
    db->dead_ids.push_back(entry_id);
    db->n_alive--;
    return MSORB_OK;
}

// (the device arrays stay reserved: the next map fills them again)
extern "C" int msorb_kf_database_clear(msorb_kf_database* db) {
    if (!db) return MSORB_E_INVALID;
    std::unique_lock<std::shared_mutex> lk(db->mu);
    db->e.clear();
    db->dead_ids.clear();
    db->n_alive = 0;
    db->rows_a = msorb::RangeAlloc();
    return MSORB_OK;
}

extern "C" int msorb_kf_database_info(const msorb_kf_database* db, int* n_entries, int* id_bound, size_t* rows_in_use, size_t* rows_reserved) {
    if (!db) return MSORB_E_INVALID;
    std::shared_lock<std::shared_mutex> lk(db->mu);
    if (n_entries) *n_entries = db->n_alive;
    if (id_bound) *id_bound = (int)db->e.size();
    if (rows_in_use) *rows_in_use = db->rows_a.end - db->rows_a.free_total();
    if (rows_reserved) *rows_reserved = db->rows_cap;
    return MSORB_OK;
}

extern "C" int msorb_kf_database_query(msorb_kf_database* db, const int* word, const double* value, int n, const uint8_t* listed, int rule,
                                       int* entry, int* common_words, double* score, int capacity, int* n_sharing, int* n_listed,
                                       int* max_common_words, int* min_common_words, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!db || n < 0 || (n > 0 && (!word || !value)) || (rule != 0 && rule != 1) || capacity < 0 ||
        (capacity > 0 && (!entry || !common_words || !score)) || !n_sharing || !n_listed || !max_common_words || !min_common_words)
        return MSORB_E_INVALID;
    if (!bow_vector_ok(word, n, db->n_words)) {
        set_last_error("kf_database_query: word ids must be strictly ascending and below n_words");
        return MSORB_E_INVALID;
    }
    std::shared_lock<std::shared_mutex> lk(db->mu);
    const int id_bound = (int)db->e.size();
    struct Hit { int first; unsigned long long seq; int id; };
    std::vector<Hit> in_list;
    std::vector<int> not_listed;
    const KfdbOut* o = nullptr;
    if (n > 0 && db->n_alive > 0) {
        // ---- staging: [query values | query words] in, [per-id results] out ----
        const size_t o_w = up16((size_t)n * 8), in_bytes = o_w + up16((size_t)n * 4), o_out = in_bytes,
                     total = o_out + (size_t)id_bound * sizeof(KfdbOut);
        static thread_local ThreadScratch scr(true, 2);
        if (int rc = scr.acquire(db->device, total, total)) return rc;
        uint8_t *const h = scr.h.p, *const d = scr.d.p;
        hipStream_t s = scr.s;
        std::memcpy(h, value, (size_t)n * 8);
        std::memcpy(h + o_w, word, (size_t)n * 4);
        // the table in LDS when a workgroup can have it: 12 B per query word, sized to this query (a relocalisation query of 300-2 000
        // words leaves room for several workgroups per CU); above 64 KB the kernel's limit has been raised once per device
        const size_t lds_bytes = (size_t)n * 12;
        const void* fn_lds = reinterpret_cast<const void*>(&kfdb_query_kernel<true>);
        bool in_lds = lds_bytes <= 64 * 1024;
        if (!in_lds) {
            const long long room = msorb::dynamic_lds_room(fn_lds);
            if (room < 0) { set_last_error("kf_database_query: the LDS limit of the kernel could not be read or raised"); return MSORB_E_HIP; }
            in_lds = (long long)lds_bytes <= room;
        }
        const int blocks = std::max(1, std::min((id_bound + kWaves - 1) / kWaves, 2048));
        hipError_t e = msorb::small_copy(d, h, in_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
        if (e == hipSuccess) {
            const double* dq_v = reinterpret_cast<const double*>(d);
            const int* dq_w = reinterpret_cast<const int*>(d + o_w);
            KfdbOut* d_out = reinterpret_cast<KfdbOut*>(d + o_out);
            if (in_lds)
                hipLaunchKernelGGL(kfdb_query_kernel<true>, dim3(blocks), dim3(kWaves * 64), lds_bytes, s, dq_w, dq_v, n, db->d_rec, id_bound,
                                   db->d_word, db->d_value, d_out);
            else
                hipLaunchKernelGGL(kfdb_query_kernel<false>, dim3(blocks), dim3(kWaves * 64), 0, s, dq_w, dq_v, n, db->d_rec, id_bound,
                                   db->d_word, db->d_value, d_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
        if (e == hipSuccess) e = msorb::small_copy(h + o_out, d + o_out, (size_t)id_bound * sizeof(KfdbOut), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
        if (e != hipSuccess) return hip_fail(scr, "kf_database_query", e);
        o = reinterpret_cast<const KfdbOut*>(h + o_out);
        for (int id = 0; id < id_bound; id++) {
            if (o[id].common <= 0) continue;
            if (!listed || listed[id]) in_list.push_back(Hit{o[id].first, db->e[id].seq, id});
            else not_listed.push_back(id);
        }
    }
    *n_sharing = (int)(in_list.size() + not_listed.size());
    if (*n_sharing > capacity) {
        set_last_error("kf_database_query: " + std::to_string(*n_sharing) + " entries share words, capacity " + std::to_string(capacity));
        return MSORB_E_CAPACITY;
    }
    // first-encounter order of the reference's walk (:612-633, :746-761): by the smallest common word, then by position in that word's list
    std::sort(in_list.begin(), in_list.end(), [](const Hit& a, const Hit& b) { return a.first != b.first ? a.first < b.first : a.seq < b.seq; });
    int max_common = 0, k = 0;
    for (const Hit& hit : in_list) {
        entry[k] = hit.id;
        common_words[k] = o[hit.id].common;
        score[k] = o[hit.id].score;
        max_common = std::max(max_common, o[hit.id].common);   // :639-644, :767-772
        k++;
    }
    for (int id : not_listed) {
        entry[k] = id;
        common_words[k] = o[id].common;
        score[k] = 0;
        k++;
    }
    *n_listed = (int)in_list.size();
    *max_common_words = max_common;
    // int * float, truncated: :774 (relocalisation), :646-650 (n-best)
    *min_common_words = rule == 0 ? (int)(max_common * 0.8f) : max_common > 10 ? (int)(max_common * 0.8f) : (int)(max_common * 0.6f);
    return MSORB_OK;
}
