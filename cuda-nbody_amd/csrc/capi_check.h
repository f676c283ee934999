// capi_check.h -- the one argument check of the extern "C" boundaries (*_capi.hip): which arrays of the caller's may reach a kernel.
// Host only, plain C++, no HIP header: tests/capi_check_test.cpp builds it with the host compiler alone.
#pragma once

#include <cstdint>
#include <initializer_list>

namespace nb {

// An array of the caller's: its address, its length in bytes, the alignment its kernel needs.  A required span that is null is
// refused; an optional span that is null is absent and takes no further part.
struct Span {
    enum Presence : bool { required, optional };
    const void*    p;
    std::uintptr_t bytes, align;
    Presence       presence = required;

    std::uintptr_t addr() const { return reinterpret_cast<std::uintptr_t>(p); }
    // absent, or there and aligned (whatever its length)
    bool sound() const { return p != nullptr ? addr() % align == 0 : presence == optional; }
    // both there, both of non-zero length, one byte or more in common
    bool overlaps(const Span& o) const {
        return p != nullptr && o.p != nullptr && bytes != 0 && o.bytes != 0 && addr() < o.addr() + o.bytes && o.addr() < addr() + bytes;
    }
};

// Every span sound; no two of `spans` overlapping, and none of `spans` overlapping one of `reads`.  The arrays a call only reads go
// into `reads` where they may alias each other (nb_field_eval_*, nb_energy_*); everywhere else every array goes into `spans`.
inline bool spans_ok(std::initializer_list<Span> spans, std::initializer_list<Span> reads = {}) {
    for (const Span& r : reads) {
        if (!r.sound()) return false;
    }
    for (const Span* x = spans.begin(); x != spans.end(); ++x) {
        if (!x->sound()) return false;
        for (const Span& r : reads) {
            if (x->overlaps(r)) return false;
        }
        for (const Span* y = x + 1; y != spans.end(); ++y) {
            if (x->overlaps(*y)) return false;
        }
    }
    return true;
}

// `rest` (which holds the array at `twin`) is fine, and `x` is the array at `twin` itself or apart from all of `rest`: the output
// of a step that may be written in place (new_positions == old_positions) or to an array of its own, and nothing in between.
inline bool in_place_or_apart(const Span& x, const void* twin, std::initializer_list<Span> rest) { return spans_ok(rest) && (x.p == twin || spans_ok({x}, rest)); }

// the sizeof_T of the nb_*_workspace_bytes queries: float or double
inline bool element_size_ok(unsigned sizeof_T) { return sizeof_T == 4 || sizeof_T == 8; }

}  // namespace nb
