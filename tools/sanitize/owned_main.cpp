// The record of a context's resources (csrc/rt_owned.h) alone, under AddressSanitizer + UndefinedBehaviorSanitizer: owned_free() is defined
// HERE, as a recorder over made-up handles, so nothing of HIP is needed.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I raytracing_simple_amd/csrc tools/sanitize/owned_main.cpp -o owned_san && ./owned_san
// One line per case ("ok <case>" / "FAILED <case>: ..."), then "owned: clean"; the exit status is the number of failed cases.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "rt_owned.h"

using rt::Owned;
using Kind = rt::Owned::Kind;

namespace {
struct Freed { Kind kind; void *handle; };
std::vector<Freed> g_freed;             // every call of owned_free, in order
std::set<void *> g_live;                // handles handed out and not yet given back
int g_double_frees = 0;                 // ... and calls for a handle that is not among them

// a made-up handle: an address nothing is stored at
char g_arena[64];
void *handle(int i) { g_live.insert(&g_arena[i]); return &g_arena[i]; }

void reset() { g_freed.clear(); g_live.clear(); g_double_frees = 0; }

int g_failed = 0;
void check(const char *name, bool ok, const char *what) {
    if (ok) printf("ok %s\n", name);
    else { printf("FAILED %s: %s\n", name, what); g_failed += 1; }
}
}  // namespace

void rt::owned_free(Kind kind, void *h) {
    g_freed.push_back(Freed{ kind, h });
    if (g_live.erase(h) == 0) g_double_frees += 1;
}

int main() {
    // the recorder itself sees a double free (what every case below relies on): one handle given back twice, on purpose
    {
        reset();
        void *h = handle(0);
        rt::owned_free(Kind::Device, h);
        rt::owned_free(Kind::Device, h);
        check("recorder_reports_a_double_free", g_double_frees == 1 && g_freed.size() == 2, "the second call for one handle was not counted");
    }
    // release(): every handle once, the last adopted first, each with its kind; the record is empty afterwards
    {
        reset();
        const Kind kinds[5] = { Kind::Stream, Kind::Event, Kind::Device, Kind::Pinned, Kind::Registered };
        void *h[5];
        Owned o;
        for (int i = 0; i < 5; ++i) o.adopt(kinds[i], h[i] = handle(i));
        o.release();
        bool ok = g_freed.size() == 5 && g_double_frees == 0 && g_live.empty() && o.size() == 0;
        for (int i = 0; ok && i < 5; ++i) ok = g_freed[i].handle == h[4 - i] && g_freed[i].kind == kinds[4 - i];
        o.release();                    // (nothing left: nothing freed)
        check("release_frees_each_once_in_reverse_with_its_kind", ok && g_freed.size() == 5, "order, kind or count");
    }
    // drop(h): given back at once, with its kind, and not again by the release() that follows; drop(null) is nothing
    {
        reset();
        void *a = handle(0), *b = handle(1), *c = handle(2);
        Owned o;
        o.adopt(Kind::Device, a);
        o.adopt(Kind::Pinned, b);
        o.adopt(Kind::Event, c);
        o.drop(nullptr);
        bool ok = g_freed.empty();
        o.drop(b);
        ok = ok && g_freed.size() == 1 && g_freed[0].handle == b && g_freed[0].kind == Kind::Pinned && o.size() == 2;
        o.release();
        ok = ok && g_freed.size() == 3 && g_freed[1].handle == c && g_freed[2].handle == a && g_double_frees == 0 && g_live.empty();
        check("drop_frees_now_and_release_not_again", ok, "a dropped handle was freed twice, late, or with another kind");
    }
    // forget(): nothing given back, nor by the destructor after it
    {
        reset();
        void *a = handle(0), *b = handle(1);
        {
            Owned o;
            o.adopt(Kind::Device, a);
            o.adopt(Kind::Stream, b);
            o.forget();
        }
        check("forget_frees_nothing_nor_the_destructor", g_freed.empty() && g_live.size() == 2, "something was freed");
    }
    // the destructor releases what is held
    {
        reset();
        void *a = handle(0), *b = handle(1);
        {
            Owned o;
            o.adopt(Kind::Device, a);
            o.adopt(Kind::Event, b);
        }
        check("destructor_releases", g_freed.size() == 2 && g_freed[0].handle == b && g_freed[1].handle == a && g_double_frees == 0 && g_live.empty(), "order or count");
    }
    // two handles exchanged between the variables that hold them (d_colors / planes.denoise after every rt_denoise_async): both once
    {
        reset();
        void *colors = handle(0), *denoise = handle(1);
        Owned o;
        o.adopt(Kind::Device, colors);
        o.adopt(Kind::Device, denoise);
        std::swap(colors, denoise);     // (the record frees by value: it never knew which variable held which)
        o.release();
        check("exchanged_handles_are_each_freed_once", g_freed.size() == 2 && g_double_frees == 0 && g_live.empty(), "a block was freed twice or not at all");
    }
    if (g_failed == 0) printf("owned: clean\n");
    return g_failed;
}
