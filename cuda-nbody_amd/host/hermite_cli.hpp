// hermite_cli.hpp -- `nbody --integrator=hermite`: the single-system run stepped by the 4th-order Hermite scheme (BodySystemHIPHermite),
// `nbody --integrator=hermite6`: the same run stepped by the 6th-order scheme (BodySystemHIPHermite6), and
// `nbody --integrator=hermite-block`: the 4th-order run with block time steps (BodySystemHIPHermiteBlock), and
// `nbody --integrator=hermite6-block`: the 6th-order run with block time steps (BodySystemHIPHermite6Block).
#pragma once

#include "nbody_types.hpp"

#include <cstddef>
#include <filesystem>
#include <vector>

struct HermiteRun {
    bool                  fp64 = false;
    std::size_t           num_bodies = 0;
    NBodyConfig           config = NBodyConfig::NBODY_CONFIG_SHELL;
    NBodyParams           params{};  // the demo row (dt, softening; its damping is not used: the scheme has none)
    bool                  benchmark = false;
    int                   iterations = 10;
    std::size_t           steps = 0;
    std::filesystem::path dump;
    bool                  energy = false;
    unsigned              knn = 0;  // --knn=<K> (0: not asked for): report_knn of the final state
    double                neighbours = -1.0;  // --neighbours=<radius> (< 0: not asked for): report_neighbours of the final state
    std::vector<double>   field_points;  // --field=<file>: x y z of every point (empty: not asked for): report_field of the final state
    bool                  sixth = false;  // --integrator=hermite6: the 6th-order scheme; with `block`: --integrator=hermite6-block
    bool                  block = false;  // --integrator=hermite-block: dt_max = the demo row's dt, `steps` / `iterations` count intervals of dt_max
    double                eta = 0.02;     // --eta (the first steps use eta_start = 0.01); hermite6-block: 0.2 unless given
    int                   levels = 30;    // --levels: steps down to dt_max * 2^-levels
};

// Starts from the current rand() state (main has applied --seed) with the single-system start-up state (the same three
// randomise_bodies segments as Compute's constructor).  --benchmark: one untimed step, then `iterations` timed ones.
auto run_hermite(const HermiteRun& run) -> void;
