// C ABI: the RCCL exchange — communicator set-up, the side stream, the row all-gathers.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstring>

#include "../../include/sah_hip.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" {

// ---- RCCL (resolved at run time so that a process which already carries an RCCL — e.g. PyTorch's — shares it) ----
// The function-pointer types come from <rccl/rccl.h> itself (decltype of the declarations), so a prototype that drifts from the
// installed library is a compile error, not a silent ABI mismatch; only the symbol lookup is deferred to dlopen / dlsym.
#define RCCL_SYM(lib, fn) reinterpret_cast<decltype(&fn)>(dlsym(lib, #fn))

static void* open_rccl() {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        void* h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) return h;
    }
    return nullptr;
}

int sah_comm_unique_id(void* out) {
    if (!out) return SAH_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(ncclUniqueId) == 128, "sah_comm_unique_id hands out 128 bytes");
    void* h = open_rccl();
    if (!h) return SAH_ERR_COMM;
    auto f = RCCL_SYM(h, ncclGetUniqueId);
    if (!f) return SAH_ERR_COMM;
    ncclUniqueId id;
    if (f(&id) != ncclSuccess) return SAH_ERR_COMM;
    memcpy(out, &id, sizeof(id));
    return SAH_OK;
}

int sah_comm_init(sah_ctx* ctx, const void* comm_id) {
    ctx->rccl = open_rccl();
    if (!ctx->rccl) return fail(ctx, SAH_ERR_COMM, "librccl not found: %s", dlerror());
    auto init = RCCL_SYM(ctx->rccl, ncclCommInitRank);
    if (!init) return fail(ctx, SAH_ERR_COMM, "ncclCommInitRank not found");
    ncclUniqueId id;
    memcpy(&id, comm_id, sizeof(id));
    if (hipSetDevice(ctx->device) != hipSuccess) return SAH_ERR_HIP;
    ncclComm_t comm = nullptr;
    const ncclResult_t rc = init(&comm, ctx->world, id, ctx->rank);
    if (rc != ncclSuccess) return fail(ctx, SAH_ERR_COMM, "ncclCommInitRank failed: %d", (int)rc);
    ctx->comm = comm;
    // The reversed-rank communicator of sah_allgather_rows_reversed is made here, while nothing is in flight on the parent (a split
    // is a collective over the parent and must not overlap its other operations).  If the installed RCCL cannot split, the reversed
    // exchange falls back to grouped point-to-point transfers on the parent communicator.
    ctx->comm_reversed = nullptr;
    // (kept: read once per communicator, selects code that ships — the send/recv fall-back for an RCCL without ncclCommSplit — and is how
    // tests/test_shard_chain.py and tests/test_comm_gpu.py reach it)
    const char* no_split = getenv("SAH_COMM_NO_SPLIT");
    auto split = RCCL_SYM(ctx->rccl, ncclCommSplit);
    ncclComm_t rev = nullptr;
    if (split && !(no_split && no_split[0] == '1')) {
        if (split(comm, 0, ctx->world - 1 - ctx->rank, &rev, nullptr) != ncclSuccess) rev = nullptr;
    }
    // Which path the reversed exchange takes must be ONE decision for the whole job: a rank on the split communicator and a rank on
    // the send / recv fallback would wait for each other forever.  So the ranks agree (minimum of "my split succeeded" over the parent
    // communicator) and the reversed communicator is used only if every rank has one.
    int mine = rev ? 1 : 0, all = 0;
    int* d_flag = nullptr;
    auto allreduce = RCCL_SYM(ctx->rccl, ncclAllReduce);
    bool agreed = false;
    if (allreduce && hipMalloc((void**)&d_flag, sizeof(int)) == hipSuccess) {
        if (hipMemcpy(d_flag, &mine, sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
            allreduce(d_flag, d_flag, 1, ncclInt32, ncclMin, comm, ctx->stream) == ncclSuccess &&
            hipStreamSynchronize(ctx->stream) == hipSuccess && hipMemcpy(&all, d_flag, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
            agreed = true;
        (void)hipFree(d_flag);
    }
    if (!agreed) {
        if (rev) {
            auto destroy = RCCL_SYM(ctx->rccl, ncclCommDestroy);
            if (destroy) destroy(rev);
        }
        return fail(ctx, SAH_ERR_COMM, "the ranks could not agree on the reversed-exchange path (ncclAllReduce on the parent communicator failed)");
    }
    if (all == 1) {
        ctx->comm_reversed = rev;
        ctx->last_error = "reversed exchange: split communicator";
    } else {
        if (rev) {
            auto destroy = RCCL_SYM(ctx->rccl, ncclCommDestroy);
            if (destroy) destroy(rev);
        }
        ctx->last_error = "reversed exchange: grouped ncclSend / ncclRecv on the parent communicator";
    }
    return SAH_OK;
}

void sah_comm_destroy(sah_ctx* ctx) {
    // nothing of this context may still be in flight on either stream when the communicators and events go away
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->rccl) {
        auto f = RCCL_SYM(ctx->rccl, ncclCommDestroy);
        if (f && ctx->comm_reversed) f((ncclComm_t)ctx->comm_reversed);
        if (f && ctx->comm) f((ncclComm_t)ctx->comm);
    }
    ctx->comm = nullptr;
    ctx->comm_reversed = nullptr;
}

int sah_comm_set_stream(sah_ctx* ctx, void* hip_stream) {
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->comm_pending) {  // a gather is still in flight on the old side stream: the work stream joins it before the streams change
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->comm_done, 0));
        ctx->comm_pending = false;
    }
    ctx->comm_stream = (hipStream_t)hip_stream;
    if (ctx->comm_stream && !ctx->comm_ready) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->comm_ready, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->comm_done, hipEventDisableTiming));
    }
    ctx->comm_pending = false;
    return SAH_OK;
}

int sah_comm_wait(sah_ctx* ctx) {
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (ctx->comm_pending) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->comm_done, 0));
        ctx->comm_pending = false;
    }
    // (what is known on the host now: a wait of an EARLIER gather that gave up.  The gather just joined may still be running; sah_sync
    // reports its outcome)
    if (sah_ipc_timed_out(ctx)) return fail(ctx, SAH_ERR_COMM, "direct exchange: a peer did not arrive within 2 s; the gathered rows are not valid");
    return SAH_OK;
}

// `reversed`: the exchange runs on a second communicator in which this process has rank world - 1 - rank (made by sah_comm_init with
// ncclCommSplit: same devices, key = reversed rank), so that the in-place slot of rank r is block world - 1 - r.  Without that
// communicator the same blocks travel as grouped ncclSend / ncclRecv pairs on the parent.
static int allgather_bytes_impl(sah_ctx* ctx, void* buffer, uint64_t bytes_per_rank, bool reversed) {
    if (!ctx || !buffer) return SAH_ERR_INVALID_ARGUMENT;
    if (bytes_per_rank == 0) return SAH_OK;
    if (const int id = sah_ipc_find(ctx, buffer, (uint64_t)ctx->world * bytes_per_rank); id >= 0) {
        // direct exchange (api_ipc.cpp): same stream discipline as the RCCL path below
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const bool side = ctx->comm_stream && ctx->comm_stream != ctx->stream;
        if (side) {
            HIP_TRY(ctx, hipEventRecord(ctx->comm_ready, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->comm_ready, 0));
            st = ctx->comm_stream;
        }
        if (int rc = sah_ipc_gather(ctx, (uint32_t)id, (uint8_t*)buffer, bytes_per_rank, reversed, st); rc != SAH_OK) return rc;
        if (side) {
            HIP_TRY(ctx, hipEventRecord(ctx->comm_done, ctx->comm_stream));
            ctx->comm_pending = true;
        }
        return SAH_OK;
    }
    if (!ctx->comm) {
        if (ctx->world == 1) return SAH_OK;  // one rank and no communicator: the buffer already is the gathered result
        return fail(ctx, SAH_ERR_COMM, "context was created without a communicator");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ncclComm_t comm = (ncclComm_t)ctx->comm;
    int slot = ctx->rank;
    const bool p2p = reversed && !ctx->comm_reversed;
    if (reversed) {
        if (ctx->comm_reversed) comm = (ncclComm_t)ctx->comm_reversed;
        slot = ctx->world - 1 - ctx->rank;
    }
    auto ag = RCCL_SYM(ctx->rccl, ncclAllGather);
    if (!ag) return fail(ctx, SAH_ERR_COMM, "ncclAllGather not found");
    const uint8_t* send = (const uint8_t*)buffer + (size_t)slot * bytes_per_rank;
    hipStream_t st = ctx->stream;
    const bool side = ctx->comm_stream && ctx->comm_stream != ctx->stream;
    if (side) {  // the gather runs behind everything enqueued so far on the work stream, and beside whatever is enqueued next
        HIP_TRY(ctx, hipEventRecord(ctx->comm_ready, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->comm_ready, 0));
        st = ctx->comm_stream;
    }
    if (p2p) {
        auto gs = RCCL_SYM(ctx->rccl, ncclGroupStart);
        auto ge = RCCL_SYM(ctx->rccl, ncclGroupEnd);
        auto snd = RCCL_SYM(ctx->rccl, ncclSend);
        auto rcv = RCCL_SYM(ctx->rccl, ncclRecv);
        if (!gs || !ge || !snd || !rcv) return fail(ctx, SAH_ERR_COMM, "ncclSend / ncclRecv / ncclGroup* not found");
        ncclResult_t rc = gs();
        for (int p = 0; p < ctx->world && rc == ncclSuccess; p++) {
            if (p == ctx->rank) continue;  // this rank's block is already in its slot
            rc = snd(send, (size_t)bytes_per_rank, ncclUint8, p, comm, st);
            if (rc == ncclSuccess) rc = rcv((uint8_t*)buffer + (size_t)(ctx->world - 1 - p) * bytes_per_rank, (size_t)bytes_per_rank, ncclUint8, p, comm, st);
        }
        const ncclResult_t rc_end = ge();
        if (rc != ncclSuccess || rc_end != ncclSuccess) return fail(ctx, SAH_ERR_COMM, "grouped ncclSend / ncclRecv failed: %d / %d", (int)rc, (int)rc_end);
    } else {
        // in place: the send buffer is this rank's slot of the receive buffer
        const ncclResult_t rc = ag(send, buffer, (size_t)bytes_per_rank, ncclUint8, comm, st);
        if (rc != ncclSuccess) return fail(ctx, SAH_ERR_COMM, "ncclAllGather failed: %d", (int)rc);
    }
    if (side) {
        HIP_TRY(ctx, hipEventRecord(ctx->comm_done, ctx->comm_stream));
        ctx->comm_pending = true;
    }
    return SAH_OK;
}

int sah_allgather_bytes(sah_ctx* ctx, void* buffer, uint64_t bytes_per_rank) { return allgather_bytes_impl(ctx, buffer, bytes_per_rank, false); }

static int allgather_rows_impl(sah_ctx* ctx, const sah_plane* image, uint32_t rows_per_rank, uint32_t allocated_rows, bool reversed) {
    if (!ctx || !image || !image->ptr) return SAH_ERR_INVALID_ARGUMENT;
    const uint64_t slots = (uint64_t)rows_per_rank * ctx->world;
    if (slots < image->height)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rows_per_rank * world = %llu leaves rows of a %u-row image ungathered", (unsigned long long)slots,
                    image->height);
    if (slots > allocated_rows)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "the allocation holds %u rows, the gather needs %llu equal slots (pad it to rows_per_rank * world)",
                    allocated_rows, (unsigned long long)slots);
    return allgather_bytes_impl(ctx, image->ptr, (uint64_t)rows_per_rank * image->row_pitch_bytes, reversed);
}

int sah_allgather_rows(sah_ctx* ctx, const sah_plane* image, uint32_t rows_per_rank, uint32_t allocated_rows) {
    SAH_RANGE();
    return allgather_rows_impl(ctx, image, rows_per_rank, allocated_rows, false);
}

int sah_allgather_rows_reversed(sah_ctx* ctx, const sah_plane* image, uint32_t rows_per_rank, uint32_t allocated_rows) {
    SAH_RANGE();
    return allgather_rows_impl(ctx, image, rows_per_rank, allocated_rows, true);
}

}  // extern "C"
