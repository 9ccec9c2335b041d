// vrccl.hip — a test-only, in-process stand-in for the RCCL calls csrc/edt_comm.cpp makes: the N
// ranks of a world are N host threads on one device (RCCL refuses two ranks on one GPU). Linked
// with the unmodified edt_comm.cpp into libedt_comm_virtual.so in place of -lrccl; the names are
// renamed by the force-included vrccl_names.h. It plays for the C schedules the role
// collectives.VirtualWorld plays for the Python ones.
//
// Semantics: exactly what include/edt_comm.h documents per collective, in-place forms included.
//   * ncclGetUniqueId makes a world record in a process-global registry; ncclCommInitRank joins it
//     and returns when all nranks ranks have joined.
//   * A collective, or a closed group (ncclGroupStart .. ncclGroupEnd: the exact schedule's K_local
//     all-to-alls, edt_comm_exchange's sends and receives), is one rendezvous of ALL ranks of the
//     world: every rank takes part in every group. Each rank records an event on the stream it
//     passed; the last rank to arrive enqueues the data movement on the world's own stream after all
//     those events, then every rank's stream is made to wait for the movement's completion.
//   * Device-to-device copies on streams only. No device-wide synchronisation and no host wait on
//     a caller's stream: a wait missing from the schedule under test is not papered over. The only
//     ordering added over RCCL's: the collectives of one world run one after the other, and a rank's
//     stream waits for the whole collective instead of for its own part of it.
//   * Reduce-scatter sums in one stated order: a left fold over ranks 0, 1, .., N-1, one fp32 add
//     per rank (fold_ranks below, compiled with -ffp-contract=off), so the reduce schedule's result
//     is a fixed function of its inputs.
//   * Where a destination overlaps a source of another rank or slice, everything of that rendezvous
//     is staged through a temporary first.
//   * Every host wait is bounded (edt_vrccl_set_wait_bound, default 30 s). A timeout, a failed
//     rank or ncclCommAbort marks the world broken: every rank waiting in it returns an error at
//     once, every later call on it returns an error, ncclCommGetAsyncError reports it.
// It shows nothing about real RCCL: transport, algorithm-dependent sum order, overlap with kernels.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "vrccl_names.h"

namespace {

constexpr int kMaxRanks = 64;
constexpr uint64_t kMagic = 0x4c43435256544445ull;   // marks a unique id made here
constexpr size_t kEventPool = 64;                    // per communicator, reused in a cycle
constexpr size_t kStageAlign = 256;

thread_local char t_err[512];
thread_local ncclResult_t t_err_code = ncclSuccess;

ncclResult_t verr(ncclResult_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
    t_err_code = code;
    return code;
}

std::atomic<double> g_bound{30.0};
std::atomic<unsigned long long> g_staged{0}, g_arrivals{0};

enum OpKind { OP_REDUCE_SCATTER, OP_ALL_GATHER, OP_ALL_TO_ALL, OP_SEND, OP_RECV };

struct VComm;

struct Op {
    OpKind kind;
    const char* send;
    char* recv;
    size_t count;      // elements per rank (collectives) or elements (point-to-point)
    size_t esz;
    int peer;
    hipStream_t stream;
    VComm* comm;
};

// What one rank brings to a rendezvous: its operations, and one recorded event per stream.
struct Slot {
    bool present = false;
    std::vector<Op> ops;
    std::vector<hipEvent_t> ready;
};

struct World {
    uint64_t id = 0;
    std::mutex mu;
    std::condition_variable cv;
    int nranks = 0;                 // set by the first rank to join
    std::vector<char> joined;
    int njoined = 0, live = 0;
    bool broken = false;
    char why[256] = "";
    uint64_t gen = 0;               // completed rendezvous
    int arrived = 0;
    std::vector<Slot> slots;
    hipStream_t stream = nullptr;   // the stand-in's own stream: all data movement of this world
    hipEvent_t done = nullptr;
    char* stage = nullptr;
    size_t stage_bytes = 0;
    std::vector<void*> old_stages;  // outgrown temporaries: possibly still in use, freed at the end
};

struct VComm {
    std::shared_ptr<World> w;
    int rank = 0;
    std::vector<hipEvent_t> pool;
    size_t next = 0;
};

std::mutex g_mu;
std::map<uint64_t, std::shared_ptr<World>> g_worlds;
uint64_t g_next_id = 1;

thread_local int t_depth = 0;
thread_local bool t_group_failed = false;
thread_local std::vector<Op> t_ops;

// w.mu held
void break_world(World& w, const char* fmt, ...) {
    if (!w.broken) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(w.why, sizeof(w.why), fmt, ap);
        va_end(ap);
        w.broken = true;
    }
    w.cv.notify_all();
}

ncclResult_t broken_error(World& w) { return verr(ncclSystemError, "virtual world broken: %s", w.why); }

std::chrono::steady_clock::time_point deadline() {
    return std::chrono::steady_clock::now() +
           std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(g_bound.load()));
}

// One communicator fewer on the world; the last one out takes the world's device resources down.
void release_world(const std::shared_ptr<World>& w) {
    bool last;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        last = --w->live == 0;
    }
    if (!last) return;
    {
        std::lock_guard<std::mutex> g(g_mu);
        g_worlds.erase(w->id);
    }
    std::lock_guard<std::mutex> lk(w->mu);
    if (!w->broken) break_world(*w, "every communicator of the world was closed");
    if (w->stream) (void)hipStreamSynchronize(w->stream);    // the stand-in's own stream only
    if (w->done) (void)hipEventDestroy(w->done);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    if (w->stage) (void)hipFree(w->stage);
    for (void* p : w->old_stages) (void)hipFree(p);
    w->done = nullptr;
    w->stream = nullptr;
    w->stage = nullptr;
    w->old_stages.clear();
}

void free_comm(VComm* c) {
    for (hipEvent_t e : c->pool) (void)hipEventDestroy(e);
    std::shared_ptr<World> w = c->w;
    delete c;
    release_world(w);
}

struct RankPtrs {
    const float* p[kMaxRanks];
};

// out[i] = ((p[0][i] + p[1][i]) + p[2][i]) + ... : the reduce-scatter's one stated order. out may
// be one of the sources (the in-place form): each element is read before it is written.
__global__ void fold_ranks(RankPtrs srcs, int nranks, float* out, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float a = srcs.p[0][i];
    for (int r = 1; r < nranks; ++r) a = a + srcs.p[r][i];
    out[i] = a;
}

struct Move {
    const char* src;
    char* dst;
    size_t bytes;
};

struct Fold {
    const char* src[kMaxRanks];
    char* dst;
    size_t count;
};

bool overlaps(const char* a, size_t na, const char* b, size_t nb) { return na && nb && a < b + nb && b < a + na; }

#define V_HIP(w, call)                                                                      \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            break_world(w, "%s: %s", #call, hipGetErrorString(e_));                         \
            return broken_error(w);                                                         \
        }                                                                                   \
    } while (0)

#define V_BAD(w, ...)               \
    do {                            \
        break_world(w, __VA_ARGS__); \
        return broken_error(w);     \
    } while (0)

// All ranks have arrived (w.mu held, by the last of them): check that their operations fit each
// other and enqueue the data movement on the world's stream after every rank's event.
ncclResult_t perform(World& w) {
    const int n = w.nranks;
    if (!w.stream) V_HIP(w, hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    if (!w.done) V_HIP(w, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    for (int r = 0; r < n; ++r)
        for (hipEvent_t e : w.slots[r].ready) V_HIP(w, hipStreamWaitEvent(w.stream, e, 0));

    std::vector<std::vector<const Op*>> coll(n), sends(n), recvs(n);
    for (int r = 0; r < n; ++r)
        for (const Op& op : w.slots[r].ops)
            (op.kind == OP_SEND ? sends : op.kind == OP_RECV ? recvs : coll)[r].push_back(&op);

    std::vector<Move> moves;
    std::vector<Fold> folds;
    for (int r = 1; r < n; ++r)
        if (coll[r].size() != coll[0].size())
            V_BAD(w, "rank %d brought %zu collectives to the rendezvous, rank 0 %zu", r, coll[r].size(), coll[0].size());
    for (size_t i = 0; i < coll[0].size(); ++i) {
        const Op& a = *coll[0][i];
        for (int r = 1; r < n; ++r) {
            const Op& b = *coll[r][i];
            if (b.kind != a.kind || b.count != a.count || b.esz != a.esz)
                V_BAD(w, "collective %zu: rank %d (kind %d, count %zu, size %zu) does not match rank 0 (kind %d, count %zu, size %zu)",
                      i, r, (int)b.kind, b.count, b.esz, (int)a.kind, a.count, a.esz);
        }
        const size_t cb = a.count * a.esz;
        if (!cb) continue;
        if (a.kind == OP_ALL_GATHER) {             // recv_q[r] = rank r's send
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < n; ++q) moves.push_back({coll[r][i]->send, coll[q][i]->recv + (size_t)r * cb, cb});
        } else if (a.kind == OP_ALL_TO_ALL) {      // recv_q[r] = rank r's send[q]
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < n; ++q)
                    moves.push_back({coll[r][i]->send + (size_t)q * cb, coll[q][i]->recv + (size_t)r * cb, cb});
        } else {                                   // recv_r = fold over q of rank q's send[r]
            for (int r = 0; r < n; ++r) {
                Fold f;
                for (int q = 0; q < n; ++q) f.src[q] = coll[q][i]->send + (size_t)r * cb;
                f.dst = coll[r][i]->recv;
                f.count = a.count;
                folds.push_back(f);
            }
        }
    }
    // point-to-point: rank d's receives from rank s pair with rank s's sends to rank d, in order
    std::vector<size_t> used(n, 0);
    std::vector<std::vector<char>> taken(n);
    for (int s = 0; s < n; ++s) taken[s].assign(sends[s].size(), 0);
    for (int d = 0; d < n; ++d) {
        for (const Op* rv : recvs[d]) {
            const int s = rv->peer;
            if (s < 0 || s >= n) V_BAD(w, "rank %d receives from rank %d of %d", d, s, n);
            size_t j = 0;
            while (j < sends[s].size() && (taken[s][j] || sends[s][j]->peer != d)) ++j;
            if (j == sends[s].size()) V_BAD(w, "rank %d receives from rank %d, which sends it nothing (more)", d, s);
            const Op* sd = sends[s][j];
            taken[s][j] = 1;
            if (sd->count * sd->esz != rv->count * rv->esz)
                V_BAD(w, "rank %d sends rank %d %zu bytes, which expects %zu", s, d, sd->count * sd->esz, rv->count * rv->esz);
            if (sd->count) moves.push_back({sd->send, rv->recv, sd->count * sd->esz});
        }
    }
    for (int s = 0; s < n; ++s)
        for (size_t j = 0; j < sends[s].size(); ++j) {
            if (sends[s][j]->peer < 0 || sends[s][j]->peer >= n)
                V_BAD(w, "rank %d sends to rank %d of %d", s, sends[s][j]->peer, n);
            if (!taken[s][j]) V_BAD(w, "rank %d sends to rank %d, which does not receive it", s, sends[s][j]->peer);
        }

    // a copy onto itself moves nothing (the owned slice of an in-place all-gather)
    size_t keep = 0;
    for (const Move& m : moves)
        if (m.src != m.dst) moves[keep++] = m;
    moves.resize(keep);

    // does any destination overlap a source it is not allowed to? (a fold may write exactly over
    // one of its own sources: the in-place reduce-scatter)
    struct Range { const char* p; size_t n; int owner; };    // owner: index of the move / fold
    std::vector<Range> srcs, dsts;
    for (size_t i = 0; i < moves.size(); ++i) {
        srcs.push_back({moves[i].src, moves[i].bytes, (int)i});
        dsts.push_back({moves[i].dst, moves[i].bytes, (int)i});
    }
    for (size_t i = 0; i < folds.size(); ++i) {
        const int id = (int)(moves.size() + i);
        for (int q = 0; q < n; ++q) srcs.push_back({folds[i].src[q], folds[i].count * 4, id});
        dsts.push_back({folds[i].dst, folds[i].count * 4, id});
    }
    bool stage = false;
    for (size_t i = 0; i < dsts.size() && !stage; ++i) {
        for (const Range& s : srcs) {
            if (!overlaps(dsts[i].p, dsts[i].n, s.p, s.n)) continue;
            const bool own_fold_source = dsts[i].owner >= (int)moves.size() && s.owner == dsts[i].owner && s.p == dsts[i].p;
            if (!own_fold_source) { stage = true; break; }
        }
        for (size_t j = 0; j < i; ++j)
            if (overlaps(dsts[i].p, dsts[i].n, dsts[j].p, dsts[j].n))
                V_BAD(w, "two destinations of one rendezvous overlap");
    }

    if (stage) {
        size_t total = 0;
        for (const Range& s : srcs) total += (s.n + kStageAlign - 1) / kStageAlign * kStageAlign;
        if (total > w.stage_bytes) {
            if (w.stage) w.old_stages.push_back(w.stage);
            w.stage = nullptr;
            w.stage_bytes = 0;
            void* p = nullptr;
            V_HIP(w, hipMalloc(&p, total));
            w.stage = static_cast<char*>(p);
            w.stage_bytes = total;
        }
        size_t off = 0;
        auto staged = [&](const char*& src, size_t bytes) -> hipError_t {
            char* t = w.stage + off;
            off += (bytes + kStageAlign - 1) / kStageAlign * kStageAlign;
            hipError_t e = hipMemcpyAsync(t, src, bytes, hipMemcpyDeviceToDevice, w.stream);
            src = t;
            return e;
        };
        for (Move& m : moves) V_HIP(w, staged(m.src, m.bytes));
        for (Fold& f : folds)
            for (int q = 0; q < n; ++q) V_HIP(w, staged(f.src[q], f.count * 4));
        g_staged += moves.size() + folds.size();
    }
    for (const Move& m : moves) V_HIP(w, hipMemcpyAsync(m.dst, m.src, m.bytes, hipMemcpyDeviceToDevice, w.stream));
    for (const Fold& f : folds) {
        RankPtrs rp;
        for (int q = 0; q < kMaxRanks; ++q) rp.p[q] = reinterpret_cast<const float*>(f.src[q < n ? q : 0]);
        const uint64_t blocks = (f.count + 255) / 256;
        if (blocks > 0x7fffffffull) V_BAD(w, "reduce-scatter of %zu elements per rank is beyond the stand-in", f.count);
        hipLaunchKernelGGL(fold_ranks, dim3((unsigned)blocks), dim3(256), 0, w.stream, rp, n,
                           reinterpret_cast<float*>(f.dst), (uint64_t)f.count);
        V_HIP(w, hipGetLastError());
    }
    V_HIP(w, hipEventRecord(w.done, w.stream));
    return ncclSuccess;
}

// One rank's part of a rendezvous: record an event per stream, deposit the operations, wait
// (bounded) for the other ranks, then make the rank's streams wait for the movement.
ncclResult_t rendezvous(VComm* c, std::vector<Op>& ops) {
    World& w = *c->w;
    ++g_arrivals;
    Slot slot;
    std::vector<hipStream_t> streams;
    for (const Op& op : ops) {
        bool seen = false;
        for (hipStream_t s : streams) seen = seen || s == op.stream;
        if (seen) continue;
        streams.push_back(op.stream);
        if (c->pool.size() < kEventPool) {
            hipEvent_t e;
            hipError_t he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (he != hipSuccess) return verr(ncclUnhandledCudaError, "hipEventCreateWithFlags: %s", hipGetErrorString(he));
            c->pool.push_back(e);
        }
        hipEvent_t ev = c->pool[c->next++ % c->pool.size()];
        hipError_t he = hipEventRecord(ev, op.stream);
        if (he != hipSuccess) {
            std::lock_guard<std::mutex> lk(w.mu);
            break_world(w, "rank %d: hipEventRecord: %s", c->rank, hipGetErrorString(he));
            return broken_error(w);
        }
        slot.ready.push_back(ev);
    }
    slot.ops = std::move(ops);
    slot.present = true;

    hipEvent_t done;
    {
        std::unique_lock<std::mutex> lk(w.mu);
        if (w.broken) return broken_error(w);
        if (w.slots[c->rank].present) {
            break_world(w, "rank %d entered a rendezvous twice (a communicator is used by one thread at a time)", c->rank);
            return broken_error(w);
        }
        w.slots[c->rank] = std::move(slot);
        const uint64_t my_gen = w.gen;
        if (++w.arrived == w.nranks) {
            ncclResult_t r = perform(w);
            for (Slot& s : w.slots) s = Slot();
            w.arrived = 0;
            if (r != ncclSuccess) return r;          // perform broke the world: the waiters return too
            ++w.gen;
            w.cv.notify_all();
        } else {
            const auto until = deadline();
            while (w.gen == my_gen && !w.broken) {
                if (w.cv.wait_until(lk, until) == std::cv_status::timeout && w.gen == my_gen && !w.broken)
                    break_world(w, "rank %d waited %.3g s at a rendezvous with %d of %d ranks present", c->rank,
                                g_bound.load(), w.arrived, w.nranks);
            }
            if (w.gen == my_gen) return broken_error(w);
        }
        done = w.done;
    }
    for (hipStream_t s : streams) {
        hipError_t he = hipStreamWaitEvent(s, done, 0);
        if (he != hipSuccess) {
            std::lock_guard<std::mutex> lk(w.mu);
            break_world(w, "rank %d: hipStreamWaitEvent: %s", c->rank, hipGetErrorString(he));
            return broken_error(w);
        }
    }
    return ncclSuccess;
}

bool elem_size(ncclDataType_t t, size_t* sz) {
    switch (t) {
        case ncclFloat32: *sz = 4; return true;
        case ncclBfloat16: *sz = 2; return true;
        case ncclUint8: *sz = 1; return true;
        default: return false;
    }
}

// A call outside a group is a group of one.
ncclResult_t submit(const Op& op) {
    if (!op.comm) return verr(ncclInvalidArgument, "null communicator");
    if (t_depth > 0) {
        t_ops.push_back(op);
        return ncclSuccess;
    }
    std::vector<Op> one{op};
    return rendezvous(op.comm, one);
}

ncclResult_t group_failure(ncclResult_t r) {
    if (r != ncclSuccess && t_depth > 0) t_group_failed = true;
    return r;
}

}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId) {
    if (!uniqueId) return verr(ncclInvalidArgument, "uniqueId is null");
    auto w = std::make_shared<World>();
    {
        std::lock_guard<std::mutex> g(g_mu);
        w->id = g_next_id++;
        g_worlds[w->id] = w;
    }
    std::memset(uniqueId, 0, sizeof(*uniqueId));
    std::memcpy(uniqueId->internal, &kMagic, 8);
    std::memcpy(uniqueId->internal + 8, &w->id, 8);
    return ncclSuccess;
}

static std::shared_ptr<World> find_world(const void* id_bytes) {
    uint64_t magic, id;
    std::memcpy(&magic, id_bytes, 8);
    std::memcpy(&id, static_cast<const char*>(id_bytes) + 8, 8);
    if (magic != kMagic) return nullptr;
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_worlds.find(id);
    return it == g_worlds.end() ? nullptr : it->second;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank) {
    if (!comm) return verr(ncclInvalidArgument, "comm is null");
    std::shared_ptr<World> w = find_world(commId.internal);
    if (!w) return verr(ncclInvalidArgument, "no live virtual world has this id");
    {
        std::unique_lock<std::mutex> lk(w->mu);
        if (w->broken) return broken_error(*w);
        if (nranks < 1 || nranks > kMaxRanks) {
            break_world(*w, "%d ranks: the stand-in takes 1..%d", nranks, kMaxRanks);
            return verr(ncclInvalidArgument, "%s", w->why);
        }
        if (w->nranks == 0) {
            w->nranks = nranks;
            w->joined.assign(nranks, 0);
            w->slots.resize(nranks);
        } else if (w->nranks != nranks) {
            break_world(*w, "rank %d joins with %d ranks, the world has %d", rank, nranks, w->nranks);
            return verr(ncclInvalidArgument, "%s", w->why);
        }
        if (rank < 0 || rank >= nranks) {
            break_world(*w, "rank %d is outside [0, %d)", rank, nranks);
            return verr(ncclInvalidArgument, "%s", w->why);
        }
        if (w->joined[rank]) {
            break_world(*w, "rank %d joined twice", rank);
            return verr(ncclInvalidArgument, "%s", w->why);
        }
        w->joined[rank] = 1;
        ++w->njoined;
        ++w->live;
        w->cv.notify_all();
        const auto until = deadline();
        while (w->njoined < w->nranks && !w->broken) {
            if (w->cv.wait_until(lk, until) == std::cv_status::timeout && w->njoined < w->nranks && !w->broken)
                break_world(*w, "rank %d waited %.3g s for the world: %d of %d ranks joined", rank, g_bound.load(),
                            w->njoined, w->nranks);
        }
        if (w->njoined < w->nranks) {
            ncclResult_t r = broken_error(*w);
            lk.unlock();
            release_world(w);
            return r;
        }
    }
    VComm* c = new VComm;
    c->w = w;
    c->rank = rank;
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    if (comm) free_comm(reinterpret_cast<VComm*>(comm));
    return ncclSuccess;
}

ncclResult_t ncclCommAbort(ncclComm_t comm) {
    if (!comm) return ncclSuccess;
    VComm* c = reinterpret_cast<VComm*>(comm);
    {
        std::lock_guard<std::mutex> lk(c->w->mu);
        break_world(*c->w, "rank %d aborted its communicator", c->rank);
    }
    free_comm(c);
    return ncclSuccess;
}

ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError) {
    if (!comm || !asyncError) return verr(ncclInvalidArgument, "null argument");
    VComm* c = reinterpret_cast<VComm*>(comm);
    std::lock_guard<std::mutex> lk(c->w->mu);
    *asyncError = c->w->broken ? broken_error(*c->w) : ncclSuccess;
    return ncclSuccess;
}

// The stand-in's own message where this thread's last failure has this code (the caller formats
// it straight into its error text), else the code's name.
const char* ncclGetErrorString(ncclResult_t result) {
    if (result != ncclSuccess && result == t_err_code && t_err[0]) return t_err;
    switch (result) {
        case ncclSuccess: return "no error";
        case ncclUnhandledCudaError: return "unhandled HIP error";
        case ncclSystemError: return "virtual world broken";
        case ncclInvalidArgument: return "invalid argument";
        case ncclInvalidUsage: return "invalid usage";
        default: return "virtual RCCL error";
    }
}

ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype,
                               ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
    if (datatype != ncclFloat32 || op != ncclSum)
        return group_failure(verr(ncclInvalidArgument, "the stand-in reduces fp32 sums only"));
    return group_failure(submit({OP_REDUCE_SCATTER, static_cast<const char*>(sendbuff), static_cast<char*>(recvbuff),
                                 recvcount, 4, -1, stream, reinterpret_cast<VComm*>(comm)}));
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                           ncclComm_t comm, hipStream_t stream) {
    size_t sz;
    if (!elem_size(datatype, &sz)) return group_failure(verr(ncclInvalidArgument, "data type %d", (int)datatype));
    return group_failure(submit({OP_ALL_GATHER, static_cast<const char*>(sendbuff), static_cast<char*>(recvbuff),
                                 sendcount, sz, -1, stream, reinterpret_cast<VComm*>(comm)}));
}

ncclResult_t ncclAllToAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                          ncclComm_t comm, hipStream_t stream) {
    size_t sz;
    if (!elem_size(datatype, &sz)) return group_failure(verr(ncclInvalidArgument, "data type %d", (int)datatype));
    return group_failure(submit({OP_ALL_TO_ALL, static_cast<const char*>(sendbuff), static_cast<char*>(recvbuff),
                                 count, sz, -1, stream, reinterpret_cast<VComm*>(comm)}));
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
    size_t sz;
    if (!elem_size(datatype, &sz)) return group_failure(verr(ncclInvalidArgument, "data type %d", (int)datatype));
    return group_failure(submit({OP_SEND, static_cast<const char*>(sendbuff), nullptr, count, sz, peer, stream,
                                 reinterpret_cast<VComm*>(comm)}));
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
    size_t sz;
    if (!elem_size(datatype, &sz)) return group_failure(verr(ncclInvalidArgument, "data type %d", (int)datatype));
    return group_failure(submit({OP_RECV, nullptr, static_cast<char*>(recvbuff), count, sz, peer, stream,
                                 reinterpret_cast<VComm*>(comm)}));
}

ncclResult_t ncclGroupStart() {
    if (t_depth++ == 0) {
        t_ops.clear();
        t_group_failed = false;
    }
    return ncclSuccess;
}

// The calls since ncclGroupStart, performed as one rendezvous. A group in which a call failed is
// dropped; an empty group is no rendezvous.
ncclResult_t ncclGroupEnd() {
    if (t_depth <= 0) return verr(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
    if (--t_depth > 0) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    if (t_group_failed) return verr(ncclInvalidUsage, "a call of this group failed; the group was dropped");
    if (ops.empty()) return ncclSuccess;
    for (const Op& op : ops)
        if (op.comm != ops[0].comm) return verr(ncclInvalidUsage, "the stand-in takes one communicator per group");
    return rendezvous(ops[0].comm, ops);
}

double edt_vrccl_set_wait_bound(double seconds) {
    if (!(seconds > 0)) return -1.0;
    return g_bound.exchange(seconds);
}

double edt_vrccl_wait_bound(void) { return g_bound.load(); }

int edt_vrccl_break_world(const void* id) {
    if (!id) return -1;
    std::shared_ptr<World> w = find_world(id);
    if (!w) return -1;
    std::lock_guard<std::mutex> lk(w->mu);
    break_world(*w, "broken by edt_vrccl_break_world");
    return 0;
}

int edt_vrccl_live_worlds(void) {
    std::lock_guard<std::mutex> g(g_mu);
    int n = 0;
    for (auto& kv : g_worlds) {
        std::lock_guard<std::mutex> lk(kv.second->mu);
        n += kv.second->live > 0;
    }
    return n;
}

unsigned long long edt_vrccl_staged_moves(void) { return g_staged.load(); }

unsigned long long edt_vrccl_arrivals(void) { return g_arrivals.load(); }

const char* edt_vrccl_last_error(void) { return t_err; }

}  // extern "C"
