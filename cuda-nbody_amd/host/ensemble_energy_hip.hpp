// ensemble_energy_hip.hpp -- EnsembleEnergyHIP<T>: the energy, momentum and angular momentum of every system of an ensemble of B systems of N
// bodies through nb_energy_ensemble_* (include/nbody_hip_energy_ensemble.h, libnbody_hip_energy_ensemble.so), and the drift since an
// earlier measurement in 64 bytes.  The workspace, the results of the last measurement, a second array for the results a drift is taken
// against and the summary record are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws
// std::runtime_error carrying the nb_error_string name.  Calls are asynchronous on `stream`; the getters wait for the null stream.
#pragma once

#include "../../include/nbody_hip_energy_ensemble.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <span>
#include <vector>

template <std::floating_point T> class EnsembleEnergyHIP {
 public:
    EnsembleEnergyHIP(std::size_t num_bodies, std::size_t num_systems) : num_bodies_(num_bodies), num_systems_(num_systems) {
        // the sizes the calls refuse are refused here, before anything is allocated
        const bool fits = num_bodies <= 0xFFFFFFFFu && num_systems <= 0xFFFFFFFFu;
        hip_check(fits ? nb_energy_ensemble_workspace_bytes(n(), b(), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT, "nb_energy_ensemble_workspace_bytes");
        workspace_ = DeviceArray<unsigned char>(workspace_bytes_);
        results_   = DeviceArray<nb_energy_t>(num_systems);
        start_     = DeviceArray<nb_energy_t>(num_systems);
        summary_   = DeviceArray<nb_energy_ensemble_drift_t>(1);
    }

    auto num_bodies() const noexcept { return num_bodies_; }
    auto num_systems() const noexcept { return num_systems_; }

    // every system of the device arrays `positions` / `velocities` (T[4*N*B] each, only read) with one softening^2 for all
    auto measure(const T* positions, const T* velocities, T softening_sq, nb_stream_t stream = nullptr) -> void {
        int status;
        if constexpr (sizeof(T) == 4) {
            status = nb_energy_ensemble_f32(positions, velocities, n(), b(), softening_sq, nullptr, 1, workspace_.data(), workspace_bytes_, results_.data(), stream);
        } else {
            status = nb_energy_ensemble_f64(positions, velocities, n(), b(), softening_sq, nullptr, 1, workspace_.data(), workspace_bytes_, results_.data(), stream);
        }
        hip_check(status, "nb_energy_ensemble");
    }

    // the B records of the last measurement
    auto results() const -> std::vector<nb_energy_t> {
        auto out = std::vector<nb_energy_t>(num_systems_);
        results_.download(out);
        return out;
    }
    auto results_device() const noexcept -> const nb_energy_t* { return results_.data(); }

    // what the last measurement says against `start`, the results() of an earlier one: folded on the device, 64 bytes read
    auto drift_since(std::span<const nb_energy_t> start, nb_stream_t stream = nullptr) -> nb_energy_ensemble_drift_t {
        start_.upload(start);
        hip_check(nb_energy_ensemble_drift(start_.data(), results_.data(), b(), summary_.data(), stream), "nb_energy_ensemble_drift");
        nb_energy_ensemble_drift_t out{};
        if (stream != nullptr) hip_check(nb_stream_synchronize(stream), "nb_stream_synchronize");
        summary_.download(std::span<nb_energy_ensemble_drift_t>(&out, 1));
        return out;
    }

 private:
    auto n() const noexcept { return static_cast<unsigned>(num_bodies_); }
    auto b() const noexcept { return static_cast<unsigned>(num_systems_); }
    std::size_t                             num_bodies_, num_systems_;
    std::size_t                             workspace_bytes_ = 0;
    DeviceArray<unsigned char>              workspace_;
    DeviceArray<nb_energy_t>                results_, start_;
    DeviceArray<nb_energy_ensemble_drift_t> summary_;
};
