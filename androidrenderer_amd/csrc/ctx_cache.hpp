// The derived device state of a context — what a launch depends on beyond its arguments — and the ONE place where the cache epoch moves.
//
// Four kinds: the two gather copies of the Lighting pass (SahLpvCopy, SahIrr32Copy), the keyed tables (SahKeyedTable: the fast kernel's column
// table, the tolerance composite's axis tables; SahTonemapCodeTables), grow-only scratch (SahBuffer) and the mip-chain generator's ticket counter
// (SahTicketCounter); and, beside them, the record of the fast Lighting kernel's strays (SahStraysRecord), which decides between two ways of
// enqueueing the same image and never moves the epoch.  Plain structs of host values and device pointers, members of sah_ctx (ctx.hpp).  An operation that can change what the NEXT identical call would enqueue takes the context's
// `cache_epoch` and raises it; nothing outside this header writes the epoch, a generation, or the extent / all-zero record of the LPV copy.
// While the epoch stands, the same call enqueues the same kernels with the same kernel arguments — what sah_chain's captured graphs rely on
// (api_chain.cpp reads it, never writes it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/sah_hip.h"
#include "params.hpp"

// (field by field: VolumeArg has four bytes of padding behind its last member, which aggregate initialisation leaves unspecified — two
// descriptors of the same volume built on different paths need not be memcmp-equal)
inline bool same_volume(const sah::VolumeArg& a, const sah::VolumeArg& b) {
    return a.ptr == b.ptr && a.width == b.width && a.height == b.height && a.depth == b.depth && a.row_pitch == b.row_pitch && a.slice_pitch == b.slice_pitch;
}

// A device buffer of the context that only grows.  Nothing happens while it holds `need` bytes; else a smaller one is freed — behind a
// synchronisation of `stream`, whose work may still use it — and a new one allocated.  `grew` (optional): a new buffer was made; what the
// owner keeps about the old one's contents (a key, a generation) is the owner's to reset.  After a failed allocation there is no buffer.
struct SahBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;

    hipError_t grow(hipStream_t stream, size_t need, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (bytes >= need) return hipSuccess;
        if (ptr) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            (void)hipFree(ptr);
        }
        ptr = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&ptr, need);
        if (e != hipSuccess) return e;
        bytes = need;
        if (grew) *grew = true;
        return hipSuccess;
    }
    // ... for a buffer whose address is a kernel argument of calls that are otherwise the same (the deferred-pixel lists of sah_lighting)
    hipError_t grow_in_epoch(hipStream_t stream, uint64_t& cache_epoch, size_t need) {
        bool grew = false;
        const hipError_t e = grow(stream, need, &grew);
        if (grew) cache_epoch++;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

// The geometry of the LPV gather copy (params.hpp: FastArgs::lpv_packed) for a volume extent
struct SahLpvPackLayout {
    uint32_t row_pitch, slice_pitch;
    uint64_t total;
};

// The Lighting pass's interleaved, zero-bordered copy of the three LPV volumes (lighting.hip).  Written whole by k_lpv_pack in front of a
// Lighting kernel, or — interior texels only — by the last step of sah_lpv_propagate; kept across calls while `generation` says so.
struct SahLpvCopy {
    SahBuffer buf;
    uint32_t generation = 0;  // sah_gi::lpv_generation the copy was built for (0: not reusable)
    sah::VolumeArg source[3] = {};
    // the volume extent whose two-texel border of the copy holds zeros ({0,0,0} + all_zero: a new allocation, zero everywhere).  The buffer is
    // grow-only and shared by every extent it is asked for: k_lpv_pack writes the border itself, the emitting propagation step writes interior
    // texels only and needs the border of ITS extent to be zero already (borders_for)
    uint32_t extent[3] = {0, 0, 0};
    bool all_zero = false;

    uint8_t* data() const { return (uint8_t*)buf.ptr; }

    static SahLpvPackLayout layout(uint32_t w, uint32_t h, uint32_t d) {
        const uint64_t row = (uint64_t)(w + 2 * sah::kLpvPackBorder) * sah::kLpvPackTexel;
        const uint64_t slice = row * (h + 2 * sah::kLpvPackBorder);
        return {(uint32_t)row, (uint32_t)slice, slice * (d + 2 * sah::kLpvPackBorder) + 64};  // + slack: the last x-pair is read as 48 bytes
    }
    // the volumes change: the copy of them is stale
    void drop(uint64_t& cache_epoch) {
        if (generation != 0) cache_epoch++;
        generation = 0;
    }
    // Room for `total` bytes.  A NEW buffer holds nothing reusable, is another kernel argument, and is zeroed on `stream`: k_lpv_pack writes the
    // border texels itself, the emitting propagation step relies on them being zero already.
    hipError_t reserve(hipStream_t stream, uint64_t& cache_epoch, uint64_t total) {
        if (buf.bytes >= total) return hipSuccess;
        const hipError_t e = buf.grow(stream, total);
        if (e != hipSuccess && buf.ptr) return e;  // (the old buffer could not be waited for: it stands, with what is known about it)
        generation = 0;
        cache_epoch++;
        if (e != hipSuccess) return e;
        extent[0] = extent[1] = extent[2] = 0;
        all_zero = true;
        return hipMemsetAsync(buf.ptr, 0, total, stream);
    }
    bool reusable_for(uint32_t gen, const sah::VolumeArg src[3]) const {
        return gen != 0 && gen == generation && same_volume(src[0], source[0]) && same_volume(src[1], source[1]) && same_volume(src[2], source[2]);
    }
    // k_lpv_pack has been enqueued for w x h x d volumes `src` under the caller's counter `gen`: interior and border of that layout are its own
    void rebuilt_by_pack(uint64_t& cache_epoch, uint32_t gen, const sah::VolumeArg src[3], uint32_t w, uint32_t h, uint32_t d) {
        if (gen != 0) cache_epoch++;  // (with 0 every call rebuilds: the same launches every time)
        generation = gen;
        for (int i = 0; i < 3; i++) source[i] = src[i];
        extent[0] = w, extent[1] = h, extent[2] = d;
        all_zero = false;
    }
    // The emitting propagation step is about to store the interior texels of a w x h x d layout: the border texels of THAT layout must hold zeros.
    // They do in a new allocation and after any writer of the same extent; a buffer last laid out for another extent (a context that lit a
    // 128 x 32 x 32 volume and now propagates three cascades: the grow-only buffer is not reallocated) holds old interior texels where the new
    // border lies — cleared here, on `stream`, ahead of the steps.
    hipError_t borders_for(hipStream_t stream, uint32_t w, uint32_t h, uint32_t d, uint64_t total) {
        const bool same = extent[0] == w && extent[1] == h && extent[2] == d;
        hipError_t e = hipSuccess;
        if (!same && !all_zero) e = hipMemsetAsync(buf.ptr, 0, total, stream);
        extent[0] = w, extent[1] = h, extent[2] = d;
        all_zero = false;
        return e;
    }
    // sah_lpv_propagate rewrites the volumes.  begin_rewrite: from here on the copy is stale, and the epoch moves WITH the drop — an early return of
    // the propagation (a failed launch, a failed reserve) leaves a dropped or half-written copy, and a captured Lighting half that reads it
    // must not be replayed.  The token keeps what the copy was.
    struct Rewrite {
        uint32_t generation;
        uint64_t epoch;
        sah::VolumeArg source[3];
    };
    Rewrite begin_rewrite(uint64_t& cache_epoch) {
        const Rewrite was = {generation, cache_epoch, {source[0], source[1], source[2]}};
        drop(cache_epoch);
        return was;
    }
    // ... and every step has been enqueued.  `last`: the three volumes the emitting step stored, whose copy it wrote — tracked from them now; null:
    // nothing was emitted, the copy stays dropped.  A frame loop that propagates into the same volumes every frame leaves the state as it found
    // it (copy tracked, made from `last`): the Lighting pass that follows enqueues what it enqueued the frame before, so the success path that
    // ends where it began takes the drop's move back.  Anything else is a change.
    void commit_rewrite(uint64_t& cache_epoch, const Rewrite& was, const sah::VolumeArg* last) {
        if (last) {
            generation = SAH_GENERATION_TRACKED;
            for (int i = 0; i < 3; i++) source[i] = last[i];
        }
        bool same = last && was.generation == SAH_GENERATION_TRACKED;
        for (int i = 0; i < 3 && same; i++) same = same_volume(was.source[i], last[i]);
        if (same && cache_epoch == was.epoch + 1) cache_epoch = was.epoch;  // (nothing but the drop has moved it: no reallocation, no other layout)
        else if (!same && last && was.generation == 0) cache_epoch++;       // a copy came into being
    }
};

// The fp32 copy of the probe irradiance atlas that the hot form of the cache gather reads (lighting_tiled.hip: k_probe_irr_unpack)
struct SahIrr32Copy {
    SahBuffer buf;
    uint32_t generation = 0;  // sah_gi::probe_generation the copy was built for (0: not reusable)
    sah::VolumeArg source = {};

    uint8_t* data() const { return (uint8_t*)buf.ptr; }

    void drop(uint64_t& cache_epoch) {  // the atlas changes: the copy of it is stale
        if (generation != 0) cache_epoch++;
        generation = 0;
    }
    hipError_t reserve(hipStream_t stream, uint64_t& cache_epoch, size_t need) {
        bool grew = false;
        const hipError_t e = buf.grow(stream, need, &grew);
        if (grew) {
            generation = 0;
            cache_epoch++;
        }
        return e;
    }
    bool reusable_for(uint32_t gen, const sah::VolumeArg& atlas) const { return gen != 0 && gen == generation && same_volume(atlas, source); }
    // k_probe_irr_unpack has been enqueued for `atlas` under the caller's counter `gen`
    void rebuilt(uint64_t& cache_epoch, uint32_t gen, const sah::VolumeArg& atlas) {
        if (gen != 0) cache_epoch++;  // (with 0 every call rebuilds: the same launches every time)
        generation = gen;
        source = atlas;
    }
    // the context tracks the copy (SAH_GENERATION_TRACKED) and made it from this very atlas: a probe update keeps it current block by block
    bool patchable_for(const sah::VolumeArg& atlas) const { return buf.ptr && generation == SAH_GENERATION_TRACKED && same_volume(atlas, source); }
};

// A device table that is a function of a few host values (the key): grown, and rebuilt by the owner's kernel when the key differs.
//     HIP_TRY(ctx, t.prepare(stream, epoch, need, key, sizeof(key), &rebuild));   if (rebuild) { launch the build; t.built(epoch, key, sizeof(key)); }
// (two calls: a build that fails to launch leaves the old key, and the epoch, alone)
struct SahKeyedTable {
    SahBuffer buf;
    uint32_t key[20] = {};
    bool valid = false;  // `key` is what the table holds (never in a new buffer)

    // `new_buffer_in_epoch`: the reallocation counts on its own, besides the rebuild that follows it (the column table of sah_lighting)
    hipError_t prepare(hipStream_t stream, uint64_t& cache_epoch, size_t need, const void* k, size_t k_bytes, bool new_buffer_in_epoch, bool* rebuild) {
        static_assert(sizeof(key) >= 7 * sizeof(float) + sizeof(uint32_t) && sizeof(key) >= 19 * sizeof(uint32_t), "the two keys in use");
        bool grew = false;
        const hipError_t e = buf.grow(stream, need, &grew);
        if (grew) {
            valid = false;
            if (new_buffer_in_epoch) cache_epoch++;
        }
        *rebuild = !valid || memcmp(k, key, k_bytes) != 0;
        return e;
    }
    void built(uint64_t& cache_epoch, const void* k, size_t k_bytes) {
        cache_epoch++;
        memcpy(key, k, k_bytes);
        valid = true;
    }
};

// The ticket counter of the mip-chain generator (mip_chain.hip): one word of device memory, made with the context so that the call
// allocates nothing.  Zero between calls: sah_mip_chain_generate zeroes it on the stream ahead of every launch and the kernel's last
// workgroup sets it back.  No launch of any other entry depends on it: it never moves the epoch.
struct SahTicketCounter {
    uint32_t* word = nullptr;

    hipError_t create() {
        const hipError_t e = hipMalloc((void**)&word, sizeof(uint32_t));
        return e != hipSuccess ? e : hipMemset(word, 0, sizeof(uint32_t));
    }
    void release() {
        if (word) (void)hipFree(word);
        word = nullptr;
    }
};

// Whether a fast Lighting launch needs the fix-up launch behind it (lighting.hip: k_lighting_fixup, which shades the pixels the fast kernel
// listed): in the frames a renderer produces nothing is listed, and the launch is a few microseconds of workgroups that read one word and
// return.  The fast kernel can finish its own strays instead (FastArgs::strays_inline) — slower where there are many, the same bytes always —
// so the launcher leaves the fix-up launch out when the recent past says there will be none:
//     the last kCleanCalls fast launches the GPU has started for this context listed nothing,
//     they were launches of the same kernel variant, width and row range as this one,
//     and the stream is not capturing (a captured call is always the two launches, and leaves this record alone: what a graph holds does not
//     depend on when it was captured, and the cache epoch has nothing to do with this).
// A launch that lists after all finishes in-kernel once; the calls behind it launch the fix-up again until kCleanCalls have been clean.
// The device half is sah::StraysRecord, in host memory the kernel stores to and `take` reads without waiting for anything, and the launch
// numbers of FrameState::call_no.  The host counts the launches it enqueues; the device's count runs ahead where captured launches are
// replayed, which `take` notices (started > issued) and takes as the end of what it knew.  No ticket, no atomic, no read-back: the record is
// a prediction, and a wrong one costs time, never a pixel.
struct SahStraysRecord {
    static constexpr uint32_t kCleanCalls = 4;
    sah::StraysRecord* rec = nullptr;  // hipHostMalloc; null after a failed allocation: the context then keeps the two launches for its whole life
    uint32_t issued = 0;     // the launch number (FrameState::call_no) the last launch enqueued outside a capture is expected to have
    uint32_t key[7] = {};    // sun mode, GI kind, pixels per thread, sky bound, width, row range of the launches numbered key_first .. issued
    uint32_t key_first = 0;
    bool have_key = false;

    // with the context, so that no call allocates (a capturing stream forbids it); a failure is not an error
    void create() {
        if (hipHostMalloc((void**)&rec, sizeof(sah::StraysRecord)) != hipSuccess) {
            (void)hipGetLastError();
            rec = nullptr;
            return;
        }
        rec->started = rec->listed = 0;
    }
    // A fast launch with key `k` is about to be enqueued, outside a capture: counts it, and tells whether it may go without the fix-up launch
    bool take(const uint32_t (&k)[7]) {
        if (!rec) return false;
        const uint32_t started = __atomic_load_n(&rec->started, __ATOMIC_RELAXED), listed = __atomic_load_n(&rec->listed, __ATOMIC_RELAXED);
        // (launch numbers are compared by their signed difference: they wrap after 2^32 launches)
        auto ahead = [](uint32_t a, uint32_t b) { return (int32_t)(a - b); };
        if (ahead(started, issued) > 0) {  // launches this record did not count have run (replays of a captured graph): of whatever extent, with whatever strays
            issued = started;
            have_key = false;
        }
        if (!have_key || memcmp(k, key, sizeof(key)) != 0) {
            memcpy(key, k, sizeof(key));
            key_first = issued + 1;
            have_key = true;
        }
        issued++;
        // launches started - kCleanCalls + 1 .. started: all of this key, none of them listed
        return ahead(started, key_first) >= (int32_t)kCleanCalls - 1 && ahead(started, listed) >= (int32_t)kCleanCalls;
    }
    void release() {
        if (rec) (void)hipHostFree(rec);
        rec = nullptr;
    }
};

// The tonemap tail's code search (api_post.cpp: ensure_tonemap_code_tables), built once per context
struct SahTonemapCodeTables {
    float* thresholds = nullptr;  // device: 256 tonemap code thresholds + the first-level bucket table
    float* code_table = nullptr;  // device: the same search as one float4 per bucket (TonemapArgs::code_table)
    uint32_t bucket_base = 0, bucket_count = 0;
    float thr_lo = 0.f, thr_hi = 0.f;

    bool ready() const { return thresholds && code_table; }
    // both tables at once: a context must not be left with one set and the other null
    void publish(uint64_t& cache_epoch, float* d_thresholds, float* d_code_table, uint32_t base, uint32_t count, float lo, float hi) {
        release();
        thresholds = d_thresholds;
        cache_epoch++;
        code_table = d_code_table;
        bucket_base = base;
        bucket_count = count;
        thr_lo = lo;
        thr_hi = hi;
    }
    void release() {
        if (thresholds) (void)hipFree(thresholds);
        if (code_table) (void)hipFree(code_table);
        thresholds = code_table = nullptr;
    }
};
