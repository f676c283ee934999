// ensemble_cli.cpp -- `nbody --systems=<B>` (ensemble_cli.hpp), and its --energies
#include "ensemble_cli.hpp"

#include "bodyensemblehip.hpp"
#include "bodyensemblehip_hermite.hpp"
#include "bodyensemblehip_hermite_block.hpp"
#include "cli_common.hpp"
#include "ensemble_energy_hip.hpp"
#include "text.hpp"

#include <algorithm>
#include <cstdio>
#include <optional>
#include <string>
#include <vector>

namespace {

// --energies: every system's energy measured on the device where the run keeps its state (EnsembleEnergyHIP), at the start and at the end;
// two lines after the run's own output.  Without the flag nothing is allocated and nothing is launched.
template <typename T> class EnergyReport {
 public:
    EnergyReport(const EnsembleRun& run, T softening_sq) : softening_sq_(softening_sq) {
        if (run.energies) meter_.emplace(run.num_bodies, run.num_systems);
    }
    template <typename Ensemble> auto start(const Ensemble& ensemble) -> void {
        if (!meter_) return;
        meter_->measure(ensemble.positions_device(), ensemble.velocities_device(), softening_sq_);
        start_ = meter_->results();
    }
    // `how_far`: "<K> steps" or "t = <T>"
    template <typename Ensemble> auto end(const Ensemble& ensemble, const std::string& how_far) -> void {
        if (!meter_) return;
        meter_->measure(ensemble.positions_device(), ensemble.velocities_device(), softening_sq_);
        const auto drift = meter_->drift_since(start_);
        auto totals = std::vector<double>();
        for (const auto& e : start_) totals.push_back(e.total);
        std::sort(totals.begin(), totals.end());
        std::printf("energies start: systems=%zu total_min=%.9g total_median=%.9g total_max=%.9g\n", start_.size(), totals.front(), totals[totals.size() / 2], totals.back());
        std::printf("energies end (%s): worst_system=%u relative_drift_max=%.9g relative_drift_rms=%.9g momentum_drift_max=%.9g not_finite=%u\n", how_far.c_str(), drift.worst_system,
                    drift.worst_relative_drift, drift.rms_relative_drift, drift.worst_momentum_drift, drift.not_finite);
    }
    static auto steps(std::size_t k) -> std::string { return std::to_string(k) + " steps"; }
    static auto time(double t) -> std::string {
        char text[48];
        std::snprintf(text, sizeof text, "t = %g", t);
        return text;
    }

 private:
    T                                   softening_sq_;
    std::optional<EnsembleEnergyHIP<T>> meter_;
    std::vector<nb_energy_t>            start_;
};

// --integrator=hermite-ensemble: --steps=K takes K fixed steps of --integrator=hermite's dt; --t-end runs the adaptive form, batches of calls
// between reads of the 64-byte status record; --benchmark times `iterations` fixed steps after one untimed, B N^2 interactions per step.
// --integrator=hermite6-ensemble is the same run at Order 6, with --integrator=hermite6's name and interaction count.
template <typename T, typename Ensemble> auto run_hermite_typed(const EnsembleRun& run, std::vector<T>& pos, std::vector<T>& vel) -> void {
    const char* const name = run.sixth ? "hermite6" : "hermite";
    const auto n = run.num_bodies, b = run.num_systems;
    // BodySystemHIP's conversions: dt float -> T, softening^2 = T(s) * T(s)
    const T dt = static_cast<T>(run.params.time_step);
    const T softening = static_cast<T>(run.params.softening), softening_sq = softening * softening;
    auto ensemble = Ensemble(n, b, softening_sq);
    ensemble.set_state(pos, vel);
    auto energies = EnergyReport<T>(run, softening_sq);
    energies.start(ensemble);
    if (run.benchmark) {
        ensemble.update(dt);  // (untimed, as Compute::run_benchmark)
        HipEvent start, stop;
        start.record();
        for (int i = 0; i < run.iterations; ++i) ensemble.update(dt);
        stop.record();
        stop.synchronize();
        const float milliseconds = HipEvent::elapsed_ms(start, stop);
        const float frequency    = static_cast<float>(run.iterations) * (1000.0f / milliseconds);
        const float interactions = static_cast<float>(static_cast<double>(b) * static_cast<double>(n) * static_cast<double>(n) * 1e-9) * frequency;
        const int   flops        = run.sixth ? 80 : 43;  // an interaction, as --integrator=hermite6 / hermite counts it
        std::printf("%zu bodies x %zu systems, %s integrator, total time for %d iterations: %s ms\n", n, b, name, run.iterations, text::width3(milliseconds).c_str());
        std::printf("= %s ms per step\n", text::width3(milliseconds / static_cast<float>(run.iterations)).c_str());
        std::printf("= %s billion interactions per second\n", text::width3(interactions).c_str());
        std::printf("= %s %s-precision GFLOP/s at %d flops per %s interaction\n", text::width3(interactions * static_cast<float>(flops)).c_str(),
                    sizeof(T) == 8 ? "double" : "single", flops, run.sixth ? "acceleration + jerk + snap" : "acceleration + jerk");
        energies.end(ensemble, energies.steps(1 + static_cast<std::size_t>(run.iterations)));
        return;
    }
    if (run.t_end > 0.0) {
        const T eta = static_cast<T>(run.eta);
        ensemble.begin(eta);
        constexpr int batch = 64;  // calls between two reads of the status record
        auto status = nb_hermite_ensemble_status_t{};
        do {
            for (int i = 0; i < batch; ++i) ensemble.advance(run.t_end, run.t_end, eta);
            status = ensemble.status();
        } while (status.done + status.stalled < status.systems && status.stepped > 0);
        auto steps = std::vector<unsigned>();
        for (const auto& clock : ensemble.clocks()) steps.push_back(clock.steps);
        std::sort(steps.begin(), steps.end());
        std::printf("%zu bodies x %zu systems, %s integrator, eta %g, to t = %g: %u systems done, %u stalled\n", n, b, name, run.eta, run.t_end, status.done, status.stalled);
        std::printf("steps per system: fewest %u, median %u, most %u; %llu in all\n", steps.front(), steps[steps.size() / 2], steps.back(), static_cast<unsigned long long>(status.total_steps));
    } else {
        for (std::size_t s = 0; s < run.steps; ++s) ensemble.update(dt);
    }
    if (!run.dump.empty()) {
        ensemble.get_positions(pos);
        ensemble.get_velocities(vel);
        write_dump<T>(run.dump, pos, vel);
    }
    energies.end(ensemble, run.t_end > 0.0 ? energies.time(run.t_end) : energies.steps(run.steps));
}

// --integrator=hermite-block-ensemble: dt_max = dt; --t-end=T (or --steps=K: T = K dt) runs every system to the last block step not past
// T, batches of calls and one summary between reads of 64 bytes; --benchmark times `iterations` intervals of dt after one untimed;
// interactions are counted as the status records count them: the sum of n_act * N over the systems.  --dump: the synchronised snapshots.
// --integrator=hermite6-block-ensemble is the same run at Order 6, with --integrator=hermite6-block's name.
template <typename T, typename Ensemble> auto run_block_typed(const EnsembleRun& run, std::vector<T>& pos, std::vector<T>& vel) -> void {
    const char* const name = run.sixth ? "hermite6-block" : "hermite-block";
    const auto   n = run.num_bodies, b = run.num_systems;
    const double dt_max = static_cast<double>(static_cast<T>(run.params.time_step));
    const T      softening = static_cast<T>(run.params.softening), softening_sq = softening * softening;
    const auto   params = nb_hermite_block_params_t{run.eta, 0.01, dt_max, run.levels, 0};
    auto         ensemble = Ensemble(n, b, softening_sq, params);
    ensemble.set_state(pos, vel);
    auto energies = EnergyReport<T>(run, softening_sq);
    if (run.energies) {
        ensemble.sync();  // (the snapshot at time 0: the state as uploaded)
        energies.start(ensemble);
    }
    const auto report = [&](const char* what, const nb_hermite_block_ensemble_summary_t& from, const nb_hermite_block_ensemble_summary_t& to) {
        const auto   body_steps  = to.body_steps - from.body_steps;
        const double evaluations = static_cast<double>(body_steps) / static_cast<double>(n);
        std::printf("%s%llu block steps, %llu body steps = %s evaluations of N^2 interactions in all, deepest level %d\n", what,
                    static_cast<unsigned long long>(to.block_steps - from.block_steps), static_cast<unsigned long long>(body_steps), text::width3(static_cast<float>(evaluations)).c_str(),
                    to.deepest_level);
    };
    if (run.benchmark) {
        const auto warm = ensemble.advance(dt_max);  // (untimed, as Compute::run_benchmark)
        HipEvent   begin, stop;
        begin.record();
        const auto end = ensemble.advance(static_cast<double>(1 + run.iterations) * dt_max);
        stop.record();
        stop.synchronize();
        const float  milliseconds = HipEvent::elapsed_ms(begin, stop);
        const double interactions = static_cast<double>(end.body_steps - warm.body_steps) * static_cast<double>(n);
        std::printf("%zu bodies x %zu systems, %s integrator, total time for %d intervals of dt_max: %s ms\n", n, b, name, run.iterations, text::width3(milliseconds).c_str());
        std::printf("= %s ms per interval\n", text::width3(milliseconds / static_cast<float>(run.iterations)).c_str());
        report("= ", warm, end);
        std::printf("= %s billion interactions per second\n", text::width3(static_cast<float>(interactions * 1e-9 / (static_cast<double>(milliseconds) * 1e-3))).c_str());
        if (run.energies) {
            ensemble.sync();
            energies.end(ensemble, energies.time(static_cast<double>(1 + run.iterations) * dt_max));
        }
        return;
    }
    const auto   none  = ensemble.summary();
    const double t_end = run.t_end > 0.0 ? run.t_end : static_cast<double>(run.steps) * dt_max;
    const auto   end   = t_end > 0.0 ? ensemble.advance(t_end) : none;
    if (!run.dump.empty()) {
        ensemble.sync();
        ensemble.get_positions(pos);
        ensemble.get_velocities(vel);
        write_dump<T>(run.dump, pos, vel);
    }
    auto steps = std::vector<unsigned long long>();
    for (const auto& status : ensemble.statuses()) steps.push_back(status.block_steps);
    std::sort(steps.begin(), steps.end());
    std::printf("%zu bodies x %zu systems, %s integrator, eta %g, %d levels, to t = %g: %u systems stopped\n", n, b, name, run.eta, run.levels, t_end, end.stopped);
    std::printf("block steps per system: fewest %llu, median %llu, most %llu\n", steps.front(), steps[steps.size() / 2], steps.back());
    report("", none, end);
    if (run.energies) {
        ensemble.sync();  // every system at its own last time not past t_end
        energies.end(ensemble, energies.time(t_end));
    }
}

// --systems without a Hermite integrator: BodyEnsembleHIP's leapfrog steps
template <typename T> auto run_plain_typed(const EnsembleRun& run, std::vector<T>& pos, std::vector<T>& vel) -> void {
    const auto n = run.num_bodies, b = run.num_systems;
    auto ensemble = BodyEnsembleHIP<T>(n, b, run.mode);
    ensemble.set_positions(pos);
    ensemble.set_velocities(vel);
    // BodySystemHIP's conversions: dt and damping float -> T, softening^2 = T(s) * T(s)
    const T dt = static_cast<T>(run.params.time_step), damping = static_cast<T>(run.params.damping);
    const T softening = static_cast<T>(run.params.softening), softening_sq = softening * softening;
    auto energies = EnergyReport<T>(run, softening_sq);
    energies.start(ensemble);
    if (run.benchmark) {
        ensemble.update(dt, damping, softening_sq);  // (untimed, as Compute::run_benchmark)
        HipEvent start, stop;
        start.record();
        for (int i = 0; i < run.iterations; ++i) ensemble.update(dt, damping, softening_sq);
        stop.record();
        stop.synchronize();
        const float milliseconds = HipEvent::elapsed_ms(start, stop);
        const float frequency    = static_cast<float>(run.iterations) * (1000.0f / milliseconds);
        const float interactions = static_cast<float>(static_cast<double>(b) * static_cast<double>(n) * static_cast<double>(n) * 1e-9) * frequency;
        const int   flops        = sizeof(T) == 8 ? 30 : 20;
        std::printf("%zu bodies x %zu systems, total time for %d iterations: %s ms\n", n, b, run.iterations, text::width3(milliseconds).c_str());
        std::printf("= %s billion interactions per second\n", text::width3(interactions).c_str());
        std::printf("= %s %s-precision GFLOP/s at %d flops per interaction\n", text::width3(interactions * static_cast<float>(flops)).c_str(), sizeof(T) == 8 ? "double" : "single", flops);
        energies.end(ensemble, energies.steps(1 + static_cast<std::size_t>(run.iterations)));
        return;
    }
    for (std::size_t s = 0; s < run.steps; ++s) ensemble.update(dt, damping, softening_sq);
    if (!run.dump.empty()) {
        ensemble.get_positions(pos);
        ensemble.get_velocities(vel);
        write_dump<T>(run.dump, pos, vel);
    }
    energies.end(ensemble, energies.steps(run.steps));
}

}  // namespace

auto run_ensemble(const EnsembleRun& run) -> void {
    with_precision_and_order(run.fp64, run.sixth, [&]<typename T, int Order>() {
        const auto n = run.num_bodies, b = run.num_systems;
        std::vector<T> pos(4 * n * b), vel(4 * n * b);
        startup_state<T>(run.config, n, b, pos, vel);
        if (run.block) {
            run_block_typed<T, BodyEnsembleHIPHermiteBlockOrder<T, Order>>(run, pos, vel);
        } else if (run.hermite) {
            run_hermite_typed<T, BodyEnsembleHIPHermiteOrder<T, Order>>(run, pos, vel);
        } else {
            run_plain_typed<T>(run, pos, vel);
        }
    });
}
