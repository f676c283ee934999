// cli_common.hpp -- what the Hermite runner (hermite_cli.cpp) and the ensemble runner (ensemble_cli.cpp) share: the start-up draws, the
// --dump file and the choice of precision and order.
#pragma once

#include "compute.hpp"
#include "randomise_bodies.hpp"

#include <cstddef>
#include <filesystem>
#include <fstream>
#include <span>
#include <stdexcept>
#include <vector>

// The start-up state of `systems` systems of n bodies from the current rand() state.  The single-system start-up state (Compute's
// constructor): an fp32 and an fp64 system reset with demo row 0's scales, then the active precision with the N-scaled ones -- that third
// segment is system 0, the next draws are systems 1 .. systems-1.
template <typename T> auto startup_state(NBodyConfig config, std::size_t n, std::size_t systems, std::span<T> pos, std::span<T> vel) -> void {
    std::vector<float>  p32(4 * n), v32(4 * n);
    std::vector<double> p64(4 * n), v64(4 * n);
    const auto demo0 = Compute::demo_params[0];
    randomise_bodies<float>(NBodyConfig::NBODY_CONFIG_SHELL, p32, v32, demo0.cluster_scale, demo0.velocity_scale);
    randomise_bodies<double>(NBodyConfig::NBODY_CONFIG_SHELL, p64, v64, demo0.cluster_scale, demo0.velocity_scale);
    auto scaled = demo0;
    Compute::scale_params_for(n, scaled);
    for (std::size_t s = 0; s < systems; ++s) {
        randomise_bodies<T>(config, pos.subspan(4 * n * s, 4 * n), vel.subspan(4 * n * s, 4 * n), scaled.cluster_scale, scaled.velocity_scale);
    }
}

// --dump: the positions, then the velocities, as they lie in memory
template <typename T> auto write_dump(const std::filesystem::path& dump, const std::vector<T>& pos, const std::vector<T>& vel) -> void {
    auto out = std::ofstream(dump, std::ios::binary | std::ios::trunc);
    if (!out) throw std::runtime_error("cannot open dump file " + dump.string());
    out.write(reinterpret_cast<const char*>(pos.data()), static_cast<std::streamsize>(pos.size() * sizeof(T)));
    out.write(reinterpret_cast<const char*>(vel.data()), static_cast<std::streamsize>(vel.size() * sizeof(T)));
}

// calls run.operator()<T, Order>() with T = double for --fp64, else float, and Order = 6 for the 6th-order integrators, else 4
template <typename Run> auto with_precision_and_order(bool fp64, bool sixth, Run&& run) -> void {
    if (fp64) {
        if (sixth) run.template operator()<double, 6>(); else run.template operator()<double, 4>();
    } else {
        if (sixth) run.template operator()<float, 6>(); else run.template operator()<float, 4>();
    }
}
