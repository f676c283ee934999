// capi_check_test.cpp -- TEST of cuda-nbody_amd/csrc/capi_check.h, the argument check of every extern "C" boundary, on a host without a GPU
// (tests/test_capi_symbols.py::test_capi_check_under_address_and_ub_sanitizers builds and runs it: -fsanitize=address,undefined, exit
// status 0 and no report).  The spans lie in one array of floats that is never read or written: only addresses are compared.
#include "../cuda-nbody_amd/csrc/capi_check.h"

#include <cstdio>

using nb::in_place_or_apart, nb::Span, nb::spans_ok;

static int failures = 0;
#define EXPECT(verdict, ...)                                            \
    do {                                                                \
        if ((__VA_ARGS__) != (verdict)) {                               \
            std::printf("line %d: expected %s\n", __LINE__, #verdict);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    alignas(16) static float pool[64];
    const std::uintptr_t     el = sizeof(float), len = 8 * el;  // arrays of 8 floats
    float* const a = pool, *const b = pool + 8, *const c = pool + 16;
    const auto   at = [&](float* p) { return Span{p, len, el}; };

    // apart (a | b | c are exactly adjacent) and aligned: fine; the order does not matter
    EXPECT(true, spans_ok({at(a), at(b), at(c)}));
    EXPECT(true, spans_ok({at(c), at(a), at(b)}));
    EXPECT(true, spans_ok({}));

    // null: a required span is refused, an optional one is absent -- whatever its length or alignment say, and next to anything
    EXPECT(false, spans_ok({at(a), {nullptr, len, el}}));
    EXPECT(false, spans_ok({{nullptr, len, el, Span::required}, at(a)}));
    EXPECT(false, spans_ok({{nullptr, 0, el}}));
    EXPECT(true, spans_ok({at(a), {nullptr, len, el, Span::optional}, at(b)}));
    EXPECT(true, spans_ok({{nullptr, ~std::uintptr_t(0), 64, Span::optional}, at(a), {nullptr, len, el, Span::optional}}));
    // an optional span that is there is a span like any other
    EXPECT(true, spans_ok({at(a), {b, len, el, Span::optional}}));
    EXPECT(false, spans_ok({at(a), {a + 7, len, el, Span::optional}}));

    // one misaligned span among aligned ones, first, in the middle and last
    const Span odd{reinterpret_cast<const char*>(c) + 1, el, el}, wide{pool + 1, el, 16};
    EXPECT(false, spans_ok({odd, at(a), at(b)}));
    EXPECT(false, spans_ok({at(a), odd, at(b)}));
    EXPECT(false, spans_ok({at(a), at(b), odd}));
    EXPECT(false, spans_ok({at(b), wide}));
    EXPECT(true, spans_ok({at(b), {pool + 4, el, 16}}));
    EXPECT(false, spans_ok({at(a), {reinterpret_cast<const char*>(c) + 1, el, el, Span::optional}}));

    // zero length: a span that is there is checked for alignment and overlaps nothing, not even from inside another
    EXPECT(true, spans_ok({at(a), {a + 3, 0, el}, {a + 3, 0, el}}));
    EXPECT(true, spans_ok({{a, 0, el}, at(a)}));
    EXPECT(false, spans_ok({at(a), {reinterpret_cast<const char*>(b) + 2, 0, el}}));
    EXPECT(true, spans_ok({at(a), {nullptr, 0, el, Span::optional}}));
    EXPECT(false, spans_ok({at(a), {nullptr, 0, el}}));

    // identical; overlapping by one element at either end; by one byte; one inside the other
    EXPECT(false, spans_ok({at(a), at(a)}));
    EXPECT(false, spans_ok({at(b), at(c), at(b)}));
    EXPECT(false, spans_ok({at(b), at(b + 7)}));
    EXPECT(false, spans_ok({at(b), at(b - 7)}));
    EXPECT(false, spans_ok({at(b + 7), at(b)}));
    EXPECT(true, spans_ok({at(b), at(b + 8), at(b - 8)}));
    EXPECT(false, spans_ok({{a, len + 1, 1}, {reinterpret_cast<const char*>(a) + len, 1, 1}}));
    EXPECT(true, spans_ok({{a, len, 1}, {reinterpret_cast<const char*>(a) + len, 1, 1}}));
    EXPECT(false, spans_ok({{a, 3 * len, el}, at(b)}));
    EXPECT(false, spans_ok({at(b), {a, 3 * len, el}}));

    // in place or apart: the array itself, shifted by one element either way, apart; the rest is checked in either case
    EXPECT(true, in_place_or_apart(at(a), a, {at(a), at(b)}));
    EXPECT(true, in_place_or_apart(at(c), a, {at(a), at(b)}));
    EXPECT(false, in_place_or_apart(at(a + 1), a, {at(a), at(c)}));
    EXPECT(false, in_place_or_apart(at(b - 1), b, {at(b), at(c)}));
    EXPECT(false, in_place_or_apart(at(b), a, {at(a), at(b)}));         // another array of the rest is not "in place"
    EXPECT(false, in_place_or_apart(at(b + 7), a, {at(a), at(c)}));     // ... nor is one that reaches into it
    EXPECT(false, in_place_or_apart(at(a), a, {at(a), at(b), at(b)}));  // the rest overlaps itself
    EXPECT(false, in_place_or_apart(at(a), a, {at(a), odd}));
    EXPECT(false, in_place_or_apart({nullptr, len, el}, nullptr, {{nullptr, len, el}, at(b)}));  // both null: the twin is required
    EXPECT(false, in_place_or_apart({nullptr, len, el}, a, {at(a), at(b)}));
    EXPECT(false, in_place_or_apart(odd, a, {at(a), at(b)}));
    EXPECT(true, in_place_or_apart(at(c), a, {at(a), {nullptr, len, el, Span::optional}}));
    EXPECT(false, in_place_or_apart(at(c), a, {at(a), {c + 7, len, el, Span::optional}}));

    // written | read: reads may alias each other; a write may touch neither a read nor another write
    EXPECT(true, spans_ok({at(c)}, {at(a), at(a), at(a + 1)}));
    EXPECT(false, spans_ok({at(a)}, {at(a), at(b)}));
    EXPECT(false, spans_ok({at(c), at(b + 7)}, {at(a)}));
    EXPECT(false, spans_ok({at(c), at(a + 7)}, {at(b)}));
    EXPECT(false, spans_ok({at(c), at(b - 7)}, {at(a)}));
    EXPECT(true, spans_ok({at(c), at(b)}, {at(a)}));
    EXPECT(false, spans_ok({at(c)}, {at(a), odd}));                    // reads are still checked for alignment
    EXPECT(false, spans_ok({at(c)}, {at(a), {nullptr, len, el}}));     // ... and for null
    EXPECT(true, spans_ok({at(c), {nullptr, len, el, Span::optional}}, {at(a), {nullptr, len, el, Span::optional}}));
    EXPECT(true, spans_ok({at(c), {a + 2, 0, 8}}, {at(a)}));  // a workspace of 0 bytes, given all the same: aligned, and in nobody's way
    EXPECT(false, spans_ok({at(c), {a + 1, 0, 8}}, {at(a)}));

    EXPECT(true, nb::element_size_ok(4) && nb::element_size_ok(8));
    EXPECT(false, nb::element_size_ok(0) || nb::element_size_ok(2) || nb::element_size_ok(16));

    if (failures == 0) std::printf("capi check ok\n");
    return failures == 0 ? 0 : 1;
}
