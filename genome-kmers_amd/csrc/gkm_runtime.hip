// gkm_runtime.hip -- the services every file of libgkm calls: device buffers (the allocator with its
// mapped-chunk path, ensure, the k-mer buffers), errors, stage timers with gk_profile_*, the small
// read-back, the lazily written enumeration.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "gkm_internal.h"

namespace gkm {

// Large device buffers (the k-mer arrays, the sort's scratch): hipMalloc, or -- GKM_VMM_CHUNK_MB=N,
// opt-in -- an address range mapped from physical allocations of N MiB each (hipMemAddressReserve /
// hipMemCreate / hipMemMap).  The scatter passes ran faster on mapped 1-4 GiB chunks: C3 69.8-70.0 ->
// 64.7-64.9 ms with 2 GiB chunks on one box (the L1 pass 18.5 -> 15.3 ms, L2 14.5 -> 13.4-13.7, the
// wave-local one 15.8 -> 15.1), 68.4 -> 64.7-65.4 ms with 1-4 GiB on another; chunks of 2-64 MiB or
// of the whole array were no better than hipMalloc (profiles/r6/ab_vmm_*.txt).  Not the default: a
// full-size C4 sort through the Python API (sort hint, prefetched class-A L0) hit an illegal address
// with it, whose cause is not found.  A failed mapping falls back to hipMalloc.
namespace {
constexpr size_t kVmmMin = 256ull << 20;  // smaller buffers: hipMalloc
struct VmmAlloc {
    size_t size, chunk;
    std::vector<hipMemGenericAllocationHandle_t> h;
};
std::mutex g_vmm_mu;
std::map<void *, VmmAlloc> g_vmm;

void vmm_release(void *base, const VmmAlloc &a) {
    for (size_t i = 0; i < a.h.size(); ++i) {
        (void)hipMemUnmap(static_cast<char *>(base) + i * a.chunk, a.chunk);
        (void)hipMemRelease(a.h[i]);
    }
    (void)hipMemAddressFree(base, a.size);
}

hipError_t vmm_alloc(void **p, size_t bytes, size_t want) {
    int dev = 0;
    hipError_t r = hipGetDevice(&dev);
    if (r != hipSuccess) return r;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    r = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
    if (r != hipSuccess) return r;
    if (gran == 0) gran = 2ull << 20;
    const size_t whole = (bytes + gran - 1) / gran * gran;
    const size_t chunk = std::min(std::max(want, gran) / gran * gran, whole);
    VmmAlloc a{(bytes + chunk - 1) / chunk * chunk, chunk, {}};
    void *base = nullptr;
    r = hipMemAddressReserve(&base, a.size, gran, nullptr, 0);
    if (r != hipSuccess) return r;
    for (size_t off = 0; off < a.size && r == hipSuccess; off += chunk) {
        hipMemGenericAllocationHandle_t h{};
        r = hipMemCreate(&h, chunk, &prop, 0);
        if (r != hipSuccess) break;
        a.h.push_back(h);
        r = hipMemMap(static_cast<char *>(base) + off, chunk, 0, h, 0);
        if (r != hipSuccess) {  // (this handle is not mapped: release it alone)
            (void)hipMemRelease(h);
            a.h.pop_back();
        }
    }
    if (r == hipSuccess) {
        hipMemAccessDesc d{};
        d.location = prop.location;
        d.flags = hipMemAccessFlagsProtReadWrite;
        r = hipMemSetAccess(base, a.size, &d, 1);
    }
    // Not filled: like hipMalloc, the contents of a new buffer are unspecified (the driver hands out
    // cleared memory either way).  A device-side zero fill here -- hipMemset or a kernel, waited for --
    // made the sorts that followed return wrong orders (test_mapped_buffers_vs_oracle: sorted by the
    // first level only, or wrong in the buffers' last chunks); no fill, or a blocking device-to-host
    // copy behind the fill, did not.  Why the filled lines go stale is not established
    if (r != hipSuccess) {
        vmm_release(base, a);
        return r;
    }
    std::lock_guard<std::mutex> g(g_vmm_mu);
    g_vmm[base] = std::move(a);
    *p = base;
    return hipSuccess;
}
}  // namespace

hipError_t dev_alloc(void **p, size_t bytes) {
    const char *e = opt("GKM_VMM_CHUNK_MB");
    const size_t want = e ? (size_t)std::strtoull(e, nullptr, 10) << 20 : 0;
    const char *tm = opt("GKM_TEST_VMM_MIN_KB");  // (tests: mapped buffers at parity-test sizes)
    const size_t vmin = tm ? (size_t)std::strtoull(tm, nullptr, 10) << 10 : kVmmMin;
    if (want == 0 || bytes < vmin) return hipMalloc(p, bytes);
    if (vmm_alloc(p, bytes, want) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();  // (the mapping's error: hipMalloc decides)
    return hipMalloc(p, bytes);
}

hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    VmmAlloc a{};
    {
        std::lock_guard<std::mutex> g(g_vmm_mu);
        auto it = g_vmm.find(p);
        if (it == g_vmm.end()) return hipFree(p);
        a = std::move(it->second);
        g_vmm.erase(it);
    }
    (void)hipDeviceSynchronize();  // (hipFree's own semantics: no kernel may still use it)
    vmm_release(p, a);
    return hipSuccess;
}

hipError_t ensure(void **p, uint64_t *cap, uint64_t bytes) {
    if (bytes == 0) bytes = 16;
    if (*p && *cap >= bytes) return hipSuccess;
    if (*p) {
        hipError_t e = dev_free(*p);
        if (e != hipSuccess) return e;
        *p = nullptr;
        *cap = 0;
    }
    hipError_t e = dev_alloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        return e;
    }
    *cap = bytes;
    return hipSuccess;
}

int fail(gk_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

int hip_fail(gk_ctx *c, hipError_t e, const char *where) {
    std::string m = std::string(hipGetErrorString(e)) + " at " + where;
    return fail(c, e == hipErrorOutOfMemory ? GK_E_OOM : GK_E_HIP, m);
}

void timer_begin(gk_ctx *c, const char *name, int *slot) {
    *slot = -1;
    if (!c->profile) return;
    Timer t;
    t.name = name;
    while (c->ev_pool.size() < c->ev_used + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->ev_pool.push_back(e);
    }
    t.start = c->ev_pool[c->ev_used++];
    t.stop = c->ev_pool[c->ev_used++];
    hipEventRecord(t.start, c->stream);
    c->timers.push_back(t);
    *slot = (int)c->timers.size() - 1;
}

void timer_end(gk_ctx *c, int slot) {
    if (slot < 0 || !c->profile) return;
    hipEventRecord(c->timers[slot].stop, c->stream);
}

void timer_units(gk_ctx *c, int slot, uint64_t units) {
    if (slot >= 0 && c->profile) c->timers[slot].units = units;
}

hipError_t read_back(gk_ctx *c, const void *dev, size_t bytes, void *host) {
    if (bytes > 8 * (size_t)kHostPinWords) return hipErrorInvalidValue;
    hipError_t e = hipMemcpyAsync(c->hpin, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) std::memcpy(host, c->hpin, bytes);
    return e;
}

// ---------------------------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------------------------
// key buffer b freed and allocated for `words` key words of elem_cap + 64 elements (contents not kept)
static int realloc_key_buffer(gk_ctx *c, int b, int words) {
    if (c->keys[b]) dev_free(c->keys[b]);
    c->keys[b] = nullptr;
    GK_TRY_HIP(c, dev_alloc(reinterpret_cast<void **>(&c->keys[b]), 8 * (uint64_t)words * (c->elem_cap + 64)));
    c->key_words_b[b] = words;
    return GK_OK;
}

int ensure_elems(gk_ctx *c, uint64_t n, int words) {
    // vals[0] / vals[1] hold data that must survive when only keys grow; grow both together
    if (n > c->elem_cap) {
        uint32_t *nv[2] = {nullptr, nullptr};
        for (int b = 0; b < 2; ++b) GK_TRY_HIP(c, dev_alloc(reinterpret_cast<void **>(&nv[b]), 4 * (n + 64)));
        if (c->have_starts && c->elem_cap > 0)
            GK_TRY_HIP(c, hipMemcpyAsync(nv[c->cur], c->vals[c->cur], 4 * c->n, hipMemcpyDeviceToDevice, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < 2; ++b) {
            if (c->vals[b]) dev_free(c->vals[b]);
            c->vals[b] = nv[b];
            if (c->keys[b]) dev_free(c->keys[b]);
            c->keys[b] = nullptr;
        }
        c->elem_cap = n;
        c->key_words_cap = 0;
        c->key_words_b[0] = c->key_words_b[1] = 0;
        c->keys_valid = c->lookup_dir_valid = false;
    }
    if (words > c->key_words_cap) {
        for (int b = 0; b < 2; ++b) {
            if (c->key_words_b[b] >= words) continue;
            if (int rc = realloc_key_buffer(c, b, words)) return rc;
        }
        c->key_words_cap = words;
        c->keys_valid = c->lookup_dir_valid = false;
    }
    const uint64_t tiles = (n + kSortTile - 1) / kSortTile + 1;
    if (tiles * 256 > c->status_cap) {
        if (c->status) hipFree(c->status);
        c->status = nullptr;
        GK_TRY_HIP(c, hipMalloc(&c->status, 8 * tiles * 256));
        GK_TRY_HIP(c, hipMemsetAsync(c->status, 0, 8 * tiles * 256, c->stream));
        c->status_cap = tiles * 256;
    }
    return GK_OK;
}

int grow_key_buffer(gk_ctx *c, int b, int words) {
    if (c->key_words_b[b] >= words) return GK_OK;
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = realloc_key_buffer(c, b, words)) return rc;
    c->key_words_cap = std::min(c->key_words_b[0], c->key_words_b[1]);
    return GK_OK;
}

int materialize_starts(gk_ctx *c) {
    if (!c->have_starts || c->starts_materialized) return GK_OK;
    int slot;
    timer_begin(c, "enumerate", &slot);
    GK_TRY_HIP(c, launch_enumerate(c, c->min_k, c->vals[c->cur]));
    timer_end(c, slot);
    c->starts_materialized = true;
    return GK_OK;
}

}  // namespace gkm

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
extern "C" int gk_profile_enable(gk_ctx *c, int on) {
    if (!c) return GK_E_ARG;
    hipStreamSynchronize(c->stream);
    c->timers.clear();
    c->ev_used = 0;
    c->profile = on != 0;
    // pre-create the events of a few hundred timed stages (a step uses tens): a timed step then
    // only records events
    while (c->profile && c->ev_pool.size() < 16384) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) break;
        c->ev_pool.push_back(e);
    }
    return GK_OK;
}

extern "C" int gk_profile_report(gk_ctx *c, char *buf, uint64_t buflen) {
    if (!c || !buf || buflen == 0) return GK_E_ARG;
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    struct Agg {
        uint64_t count = 0, units = 0;
        double ms = 0;
    };
    std::map<std::string, Agg> agg;
    for (auto &t : c->timers) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
            auto &a = agg[t.name];
            a.count += 1;
            a.ms += ms;
            a.units += t.units;
        }
    }
    std::string s = "{";
    bool first = true;
    for (auto &kv : agg) {
        char tmp[320];
        std::snprintf(tmp, sizeof tmp, "%s\"%s\": {\"count\": %llu, \"total_ms\": %.6f, \"units\": %llu}",
                      first ? "" : ", ", kv.first.c_str(), (unsigned long long)kv.second.count, kv.second.ms,
                      (unsigned long long)kv.second.units);
        s += tmp;
        first = false;
    }
    s += "}";
    std::snprintf(buf, (size_t)buflen, "%s", s.c_str());
    return s.size() < buflen ? GK_OK : GK_E_ARG;
}
