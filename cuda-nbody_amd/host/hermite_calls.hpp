// hermite_calls.hpp -- the C functions of the eight Hermite libraries (include/nbody_hip_hermite*.h), named once.  One table per
// shape (solo, block, ensemble, block ensemble), specialised by order; the precision picks _f32 or _f64 inside it.  An entry is the
// function's address and the name hip_check puts into the error message, both compile-time constants: a wrapper calls
// `Calls::step.fn(...)` and reports `Calls::step.name`.  The 4th- and 6th-order functions of a shape differ in their argument lists
// (the snaps and crackles), so the wrappers choose the list by `Order` where they call.
#pragma once

#include "../../include/nbody_hip_hermite.h"
#include "../../include/nbody_hip_hermite6.h"
#include "../../include/nbody_hip_hermite6_block.h"
#include "../../include/nbody_hip_hermite6_block_ensemble.h"
#include "../../include/nbody_hip_hermite6_ensemble.h"
#include "../../include/nbody_hip_hermite_block.h"
#include "../../include/nbody_hip_hermite_block_ensemble.h"
#include "../../include/nbody_hip_hermite_ensemble.h"

#include <concepts>

template <typename F> struct HermiteCall {
    F*          fn;
    const char* name;
};
template <typename F> HermiteCall(F*, const char*) -> HermiteCall<F>;

template <std::floating_point T, typename F32, typename F64> constexpr auto by_precision(F32* f32, F64* f64) noexcept {
    if constexpr (sizeof(T) == 4) return f32; else return f64;
}

// one system: BodySystemHIPHermiteOrder (bodysystemhip_hermite.hpp)
template <std::floating_point T, int Order> struct HermiteCalls;
template <std::floating_point T> struct HermiteCalls<T, 4> {
    static constexpr HermiteCall workspace_bytes{nb_hermite_workspace_bytes, "nb_hermite_workspace_bytes"};
    static constexpr HermiteCall eval{by_precision<T>(nb_hermite_eval_f32, nb_hermite_eval_f64), "nb_hermite_eval"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite_step_f32, nb_hermite_step_f64), "nb_hermite_step"};
};
template <std::floating_point T> struct HermiteCalls<T, 6> {
    static constexpr HermiteCall workspace_bytes{nb_hermite6_workspace_bytes, "nb_hermite6_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite6_init_f32, nb_hermite6_init_f64), "nb_hermite6_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite6_step_f32, nb_hermite6_step_f64), "nb_hermite6_step"};
};

// one system, block time steps: BodySystemHIPHermiteBlockOrder (bodysystemhip_hermite_block.hpp)
template <std::floating_point T, int Order> struct HermiteBlockCalls;
template <std::floating_point T> struct HermiteBlockCalls<T, 4> {
    static constexpr HermiteCall workspace_bytes{nb_hermite_block_workspace_bytes, "nb_hermite_block_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite_block_init_f32, nb_hermite_block_init_f64), "nb_hermite_block_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite_block_step_f32, nb_hermite_block_step_f64), "nb_hermite_block_step"};
    static constexpr HermiteCall sync{by_precision<T>(nb_hermite_block_sync_f32, nb_hermite_block_sync_f64), "nb_hermite_block_sync"};
};
template <std::floating_point T> struct HermiteBlockCalls<T, 6> {
    static constexpr HermiteCall workspace_bytes{nb_hermite6_block_workspace_bytes, "nb_hermite6_block_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite6_block_init_f32, nb_hermite6_block_init_f64), "nb_hermite6_block_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite6_block_step_f32, nb_hermite6_block_step_f64), "nb_hermite6_block_step"};
    static constexpr HermiteCall sync{by_precision<T>(nb_hermite6_block_sync_f32, nb_hermite6_block_sync_f64), "nb_hermite6_block_sync"};
};

// many systems: BodyEnsembleHIPHermiteOrder (bodyensemblehip_hermite.hpp)
template <std::floating_point T, int Order> struct HermiteEnsembleCalls;
template <std::floating_point T> struct HermiteEnsembleCalls<T, 4> {
    static constexpr HermiteCall workspace_bytes{nb_hermite_ensemble_workspace_bytes, "nb_hermite_ensemble_workspace_bytes"};
    static constexpr HermiteCall eval{by_precision<T>(nb_hermite_ensemble_eval_f32, nb_hermite_ensemble_eval_f64), "nb_hermite_ensemble_eval"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite_ensemble_step_f32, nb_hermite_ensemble_step_f64), "nb_hermite_ensemble_step"};
    static constexpr HermiteCall begin{by_precision<T>(nb_hermite_ensemble_begin_f32, nb_hermite_ensemble_begin_f64), "nb_hermite_ensemble_begin"};
    static constexpr HermiteCall advance{by_precision<T>(nb_hermite_ensemble_advance_f32, nb_hermite_ensemble_advance_f64), "nb_hermite_ensemble_advance"};
};
template <std::floating_point T> struct HermiteEnsembleCalls<T, 6> {
    static constexpr HermiteCall workspace_bytes{nb_hermite6_ensemble_workspace_bytes, "nb_hermite6_ensemble_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite6_ensemble_init_f32, nb_hermite6_ensemble_init_f64), "nb_hermite6_ensemble_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite6_ensemble_step_f32, nb_hermite6_ensemble_step_f64), "nb_hermite6_ensemble_step"};
    static constexpr HermiteCall begin{by_precision<T>(nb_hermite6_ensemble_begin_f32, nb_hermite6_ensemble_begin_f64), "nb_hermite6_ensemble_begin"};
    static constexpr HermiteCall advance{by_precision<T>(nb_hermite6_ensemble_advance_f32, nb_hermite6_ensemble_advance_f64), "nb_hermite6_ensemble_advance"};
};

// many systems, block time steps: BodyEnsembleHIPHermiteBlockOrder (bodyensemblehip_hermite_block.hpp)
template <std::floating_point T, int Order> struct HermiteBlockEnsembleCalls;
template <std::floating_point T> struct HermiteBlockEnsembleCalls<T, 4> {
    static constexpr HermiteCall workspace_bytes{nb_hermite_block_ensemble_workspace_bytes, "nb_hermite_block_ensemble_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite_block_ensemble_init_f32, nb_hermite_block_ensemble_init_f64), "nb_hermite_block_ensemble_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite_block_ensemble_step_f32, nb_hermite_block_ensemble_step_f64), "nb_hermite_block_ensemble_step"};
    static constexpr HermiteCall sync{by_precision<T>(nb_hermite_block_ensemble_sync_f32, nb_hermite_block_ensemble_sync_f64), "nb_hermite_block_ensemble_sync"};
    static constexpr HermiteCall summary{nb_hermite_block_ensemble_summary, "nb_hermite_block_ensemble_summary"};
};
template <std::floating_point T> struct HermiteBlockEnsembleCalls<T, 6> {
    static constexpr HermiteCall workspace_bytes{nb_hermite6_block_ensemble_workspace_bytes, "nb_hermite6_block_ensemble_workspace_bytes"};
    static constexpr HermiteCall init{by_precision<T>(nb_hermite6_block_ensemble_init_f32, nb_hermite6_block_ensemble_init_f64), "nb_hermite6_block_ensemble_init"};
    static constexpr HermiteCall step{by_precision<T>(nb_hermite6_block_ensemble_step_f32, nb_hermite6_block_ensemble_step_f64), "nb_hermite6_block_ensemble_step"};
    static constexpr HermiteCall sync{by_precision<T>(nb_hermite6_block_ensemble_sync_f32, nb_hermite6_block_ensemble_sync_f64), "nb_hermite6_block_ensemble_sync"};
    static constexpr HermiteCall summary{nb_hermite6_block_ensemble_summary, "nb_hermite6_block_ensemble_summary"};
};
