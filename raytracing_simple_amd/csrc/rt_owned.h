// rt_owned.h -- the record of what a context has taken from the runtime: device blocks, page-locked host blocks, a caller's host range
// it registered, events, streams -- one entry per handle, in order of acquisition.  Whoever acquires a handle enters it here (the typed
// helpers of rt_internal.h do both at once); teardown is release(), which gives everything back in reverse order, or forget(), which
// gives nothing back -- the context whose streams may hold work that never completes.  The members that hold the handles (rt_ctx,
// rt_multi) stay raw pointers: the record frees by value, so exchanging two of them (d_colors / planes.denoise) needs nothing here.
// No HIP in here -- giving back goes through owned_free(), which rt_api.hip defines; tools/sanitize/owned_main.cpp defines its own
// and drives the record with the host compiler alone.
#pragma once

#include <cassert>
#include <cstddef>
#include <vector>

namespace rt {

struct Owned {
    enum class Kind : unsigned char { Device, Pinned, Registered, Event, Stream };

    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { release(); }

    void adopt(Kind kind, void *handle) { held.push_back(Entry{ kind, handle }); }

    // one handle given back now (a buffer that is replaced by a larger one).  Null: nothing; a handle the record does not hold is a programming error
    void drop(void *handle);

    // everything given back, the last acquired first: the context's stream is its first acquisition and so goes last
    void release();

    // nothing given back: the handles are leaked on purpose
    void forget() { held.clear(); }

    size_t size() const { return held.size(); }

private:
    struct Entry { Kind kind; void *handle; };
    std::vector<Entry> held;
};

// the one place a handle goes back to the runtime; whatever the runtime answers is discarded
void owned_free(Owned::Kind kind, void *handle);

inline void Owned::drop(void *handle) {
    if (!handle) return;
    for (size_t i = held.size(); i-- > 0;)
        if (held[i].handle == handle) {
            const Kind kind = held[i].kind;
            held.erase(held.begin() + (std::ptrdiff_t)i);
            owned_free(kind, handle);
            return;
        }
    assert(!"rt::Owned::drop: a handle the record does not hold");
}

inline void Owned::release() {
    while (!held.empty()) {
        const Entry e = held.back();
        held.pop_back();
        owned_free(e.kind, e.handle);
    }
}

}  // namespace rt
