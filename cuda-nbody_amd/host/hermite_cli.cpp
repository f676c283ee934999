// hermite_cli.cpp -- `nbody --integrator=hermite`, `hermite6`, `hermite-block` and `hermite6-block` (hermite_cli.hpp)
#include "hermite_cli.hpp"

#include "bodysystemhip_hermite.hpp"
#include "bodysystemhip_hermite_block.hpp"
#include "cli_common.hpp"
#include "field_cli.hpp"
#include "knn_cli.hpp"
#include "neighbour_cli.hpp"
#include "text.hpp"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace {

// nb_energy_* of the product library on the system's arrays (softening^2 is that library's process-global setting)
template <typename System, typename T> auto energy_of(const System& system, T softening_sq) -> nb_energy_t {
    const auto  n     = static_cast<unsigned>(system.num_bodies());
    std::size_t bytes = 0;
    hip_check(nb_energy_workspace_bytes(n, &bytes), "nb_energy_workspace_bytes");
    auto workspace = DeviceArray<unsigned char>(bytes);
    auto result    = DeviceArray<nb_energy_t>(1);
    if constexpr (sizeof(T) == 4) {
        hip_check(nb_set_softening_sq_f32(softening_sq), "nb_set_softening_sq_f32");
        hip_check(nb_energy_f32(system.positions(), system.velocities(), n, workspace.data(), bytes, result.data(), nullptr), "nb_energy_f32");
    } else {
        hip_check(nb_set_softening_sq_f64(softening_sq), "nb_set_softening_sq_f64");
        hip_check(nb_energy_f64(system.positions(), system.velocities(), n, workspace.data(), bytes, result.data(), nullptr), "nb_energy_f64");
    }
    nb_energy_t out{};
    result.download(std::span<nb_energy_t>(&out, 1));
    return out;
}

auto print_energy(const std::string& what, const nb_energy_t& e) -> void {
    std::printf("%s: kinetic=%.9g potential=%.9g total=%.9g momentum=%.9g,%.9g,%.9g", what.c_str(), e.kinetic, e.potential, e.total, e.momentum[0], e.momentum[1], e.momentum[2]);
}

// What a run reports besides its own lines, of the fixed-step and of the block systems alike: --energy (measured at construction, after
// set_state, and again by energy()), --neighbours, --knn and --field of the present state.  A block system is synchronised first: each
// report reads its snapshot.
template <typename T, typename System> class Reports {
 public:
    Reports(const HermiteRun& run, System& system, std::vector<T>& pos, T softening_sq)
        : run_(run), system_(system), pos_(pos), softening_sq_(softening_sq), measure_(run.energy && (run.benchmark || run.steps > 0)) {
        if (!measure_) return;
        snapshot();
        start_ = energy_of(system_, softening_sq_);
    }
    auto energy(std::size_t steps) -> void {
        if (!measure_) return;
        snapshot();
        const auto end = energy_of(system_, softening_sq_);
        print_energy("energy start", start_);
        std::printf("\n");
        print_energy("energy end (" + std::to_string(steps) + " steps)", end);
        std::printf(" relative_drift=%.9g\n", (end.total - start_.total) / std::abs(start_.total));
    }
    auto neighbourhood() -> void {
        if (run_.neighbours < 0) return;
        report_neighbours(positions(), run_.neighbours, softening_sq_);
    }
    auto structure() -> void {
        if (run_.knn == 0) return;
        report_knn(positions(), run_.knn);
    }
    auto field_points() -> void {
        if (run_.field_points.empty()) return;
        report_field(positions(), run_.field_points, softening_sq_);
    }

 private:
    auto snapshot() -> void {
        if constexpr (requires { system_.sync(); }) system_.sync();
    }
    auto positions() -> std::span<const T> {
        snapshot();
        system_.get_positions(pos_);
        return pos_;
    }
    const HermiteRun& run_;
    System&           system_;
    std::vector<T>&   pos_;
    T                 softening_sq_;
    bool              measure_;
    nb_energy_t       start_{};
};

// what --benchmark prints of a scheme: its name, the flops of one interaction as its library evaluates it, and what the interaction returns
struct Scheme {
    const char* name;
    int         flops;
    const char* interaction;
};
// an acceleration + jerk interaction: 3 + 3 subtractions, 2 x 5 for r.r + eps^2 and r.w, rsqrt (4, the reference's convention), 2 + 1
// products for s^-2, s^-3 and the mass, 2 for -3 (r.w) s^-2, 6 + 12 for the two sums
constexpr Scheme kHermite4{"hermite", 43, "acceleration + jerk"};
// an acceleration + jerk + snap interaction, counted the same way: 9 subtractions, 5 + 5 + 11 for r.r + eps^2, r.w and w.w + r.b, rsqrt (4),
// 2 + 1 products for s^-2, s^-3 and the mass, 7 for alpha, beta and their multiples by -3 and -6, 6 + 12 + 18 for the three sums
constexpr Scheme kHermite6{"hermite6", 80, "acceleration + jerk + snap"};
// the block integrators: hermite-block prints no FLOP line (its output is what it was); hermite6-block counts hermite6's interaction
constexpr Scheme kHermiteBlock{"hermite-block", 0, "acceleration + jerk"};
constexpr Scheme kHermite6Block{"hermite6-block", kHermite6.flops, kHermite6.interaction};

// --integrator=hermite-block and hermite6-block: dt_max = dt, --steps=K advances to K dt, --benchmark times `iterations` intervals of dt after
// one untimed; interactions are counted as the status record counts them: sum of n_act * N
template <typename T, typename System> auto run_block_typed(const HermiteRun& run, const Scheme& scheme) -> void {
    const auto     n = run.num_bodies;
    std::vector<T> pos(4 * n), vel(4 * n);
    startup_state<T>(run.config, n, 1, pos, vel);
    const double dt_max = static_cast<double>(static_cast<T>(run.params.time_step));
    const T      softening = static_cast<T>(run.params.softening), softening_sq = softening * softening;
    const auto   params = nb_hermite_block_params_t{run.eta, 0.01, dt_max, run.levels, 0};
    auto         system = System(n, softening_sq, params);
    system.set_state(pos, vel);
    auto reports = Reports<T, System>(run, system, pos, softening_sq);
    const auto report = [&](const char* what, const nb_hermite_block_status_t& from, const nb_hermite_block_status_t& to) {
        const auto   body_steps = to.body_steps - from.body_steps;
        const double evaluations = static_cast<double>(body_steps) / static_cast<double>(n);
        std::printf("%s%llu block steps, %llu body steps = %s evaluations of N^2 interactions, deepest level %d\n", what, static_cast<unsigned long long>(to.block_steps - from.block_steps),
                    static_cast<unsigned long long>(body_steps), text::width3(static_cast<float>(evaluations)).c_str(), to.deepest_level);
    };
    if (run.benchmark) {
        const auto warm = system.advance(dt_max);  // (untimed, as Compute::run_benchmark)
        HipEvent   begin, stop;
        begin.record();
        const auto end = system.advance(static_cast<double>(1 + run.iterations) * dt_max);
        stop.record();
        stop.synchronize();
        const float  milliseconds = HipEvent::elapsed_ms(begin, stop);
        const double interactions = static_cast<double>(end.body_steps - warm.body_steps) * static_cast<double>(n);
        std::printf("%zu bodies, %s integrator, total time for %d intervals of dt_max: %s ms\n", n, scheme.name, run.iterations, text::width3(milliseconds).c_str());
        std::printf("= %s ms per interval\n", text::width3(milliseconds / static_cast<float>(run.iterations)).c_str());
        report("= ", warm, end);
        const auto per_second = static_cast<float>(interactions * 1e-9 / (static_cast<double>(milliseconds) * 1e-3));
        std::printf("= %s billion interactions per second\n", text::width3(per_second).c_str());
        if (scheme.flops > 0) {
            std::printf("= %s %s-precision GFLOP/s at %d flops per %s interaction\n", text::width3(per_second * static_cast<float>(scheme.flops)).c_str(),
                        sizeof(T) == 8 ? "double" : "single", scheme.flops, scheme.interaction);
        }
        reports.energy(1 + static_cast<std::size_t>(run.iterations));
        reports.neighbourhood();
        reports.field_points();
        return;
    }
    const auto none = system.status();
    const auto end  = run.steps > 0 ? system.advance(static_cast<double>(run.steps) * dt_max) : none;
    if (!run.dump.empty()) {
        system.sync();
        system.get_positions(pos);
        system.get_velocities(vel);
        write_dump<T>(run.dump, pos, vel);
    }
    report("", none, end);
    reports.energy(run.steps);
    reports.neighbourhood();
    reports.structure();
    reports.field_points();
}

template <typename T, typename System> auto run_typed(const HermiteRun& run, const Scheme& scheme) -> void {
    const auto     n = run.num_bodies;
    std::vector<T> pos(4 * n), vel(4 * n);
    startup_state<T>(run.config, n, 1, pos, vel);
    // BodySystemHIP's conversions: dt float -> T, softening^2 = T(s) * T(s)
    const T dt = static_cast<T>(run.params.time_step);
    const T softening = static_cast<T>(run.params.softening), softening_sq = softening * softening;
    auto system = System(n, softening_sq);
    system.set_state(pos, vel);
    auto reports = Reports<T, System>(run, system, pos, softening_sq);
    if (run.benchmark) {
        system.update(dt);  // (untimed, as Compute::run_benchmark)
        HipEvent begin, stop;
        begin.record();
        for (int i = 0; i < run.iterations; ++i) system.update(dt);
        stop.record();
        stop.synchronize();
        const float milliseconds = HipEvent::elapsed_ms(begin, stop);
        const float frequency    = static_cast<float>(run.iterations) * (1000.0f / milliseconds);
        const float interactions = static_cast<float>(static_cast<double>(n) * static_cast<double>(n) * 1e-9) * frequency;
        const int flops = scheme.flops;
        std::printf("%zu bodies, %s integrator, total time for %d iterations: %s ms\n", n, scheme.name, run.iterations, text::width3(milliseconds).c_str());
        std::printf("= %s ms per step\n", text::width3(milliseconds / static_cast<float>(run.iterations)).c_str());
        std::printf("= %s billion interactions per second\n", text::width3(interactions).c_str());
        std::printf("= %s %s-precision GFLOP/s at %d flops per %s interaction\n", text::width3(interactions * static_cast<float>(flops)).c_str(),
                    sizeof(T) == 8 ? "double" : "single", flops, scheme.interaction);
        reports.energy(1 + static_cast<std::size_t>(run.iterations));
        reports.neighbourhood();
        reports.field_points();
        return;
    }
    for (std::size_t s = 0; s < run.steps; ++s) system.update(dt);
    if (!run.dump.empty()) {
        system.get_positions(pos);
        system.get_velocities(vel);
        write_dump<T>(run.dump, pos, vel);
    }
    reports.energy(run.steps);
    reports.neighbourhood();
    reports.structure();
    reports.field_points();
}

}  // namespace

auto run_hermite(const HermiteRun& run) -> void {
    with_precision_and_order(run.fp64, run.sixth, [&]<typename T, int Order>() {
        if (run.block) {
            run_block_typed<T, BodySystemHIPHermiteBlockOrder<T, Order>>(run, Order == 6 ? kHermite6Block : kHermiteBlock);
        } else {
            run_typed<T, BodySystemHIPHermiteOrder<T, Order>>(run, Order == 6 ? kHermite6 : kHermite4);
        }
    });
}
