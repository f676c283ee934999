// field_hip.hpp -- FieldProbeHIP<T>: acceleration, jerk and potential of N sources at M points of the caller's own through
// nb_field_eval_* (include/nbody_hip_field.h, libnbody_hip_field.so).  The outputs, the workspace and staging copies of the inputs are
// DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws std::runtime_error carrying the nb_error_string
// name.  Calls are asynchronous on `stream`; the getters wait for the null stream.
#pragma once

#include "../../include/nbody_hip_field.h"
#include "device_array.hpp"

#include <algorithm>
#include <concepts>
#include <cstddef>
#include <span>

template <std::floating_point T> class FieldProbeHIP {
 public:
    FieldProbeHIP(std::size_t num_sources, std::size_t num_targets) : num_sources_(num_sources), num_targets_(num_targets) {
        // the sizes the calls refuse are refused here, before anything is allocated
        const bool fits = num_sources <= 0xFFFFFFFFu && num_targets <= 0xFFFFFFFFu;
        hip_check(fits ? nb_field_workspace_bytes(static_cast<unsigned>(num_sources), static_cast<unsigned>(num_targets), sizeof(T), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT,
                  "nb_field_workspace_bytes");
        sources_    = DeviceArray<T>(4 * num_sources);
        targets_    = DeviceArray<T>(4 * num_targets);
        acc_        = DeviceArray<T>(4 * num_targets);
        potentials_ = DeviceArray<T>(num_targets);
        workspace_  = DeviceArray<unsigned char>(std::max<std::size_t>(workspace_bytes_, 256));
    }

    auto num_sources() const noexcept { return num_sources_; }
    auto num_targets() const noexcept { return num_targets_; }

    // accelerations and potentials of the device arrays `sources` (T[4 N]) at `targets` (T[4 M]); self_index (unsigned[M]) may be null
    auto eval(const T* sources, const T* targets, const unsigned* self_index, T softening_sq, nb_stream_t stream = nullptr) -> void {
        const auto n = static_cast<unsigned>(num_sources_), m = static_cast<unsigned>(num_targets_);
        int        status;
        if constexpr (sizeof(T) == 4) {
            status = nb_field_eval_f32(sources, nullptr, n, targets, nullptr, self_index, m, softening_sq, acc_.data(), nullptr, potentials_.data(), workspace_.data(),
                                       workspace_.size(), stream);
        } else {
            status = nb_field_eval_f64(sources, nullptr, n, targets, nullptr, self_index, m, softening_sq, acc_.data(), nullptr, potentials_.data(), workspace_.data(),
                                       workspace_.size(), stream);
        }
        hip_check(status, "nb_field_eval");
    }
    // ... of a state and points on the host; nobody is excluded
    auto eval(std::span<const T> sources, std::span<const T> targets, T softening_sq) -> void {
        sources_.upload(sources);
        targets_.upload(targets);
        eval(sources_.data(), targets_.data(), nullptr, softening_sq);
    }

    auto get_accelerations(std::span<T> out) const -> void { acc_.download(out); }
    auto get_potentials(std::span<T> out) const -> void { potentials_.download(out); }

 private:
    std::size_t                num_sources_, num_targets_;
    std::size_t                workspace_bytes_ = 0;
    DeviceArray<T>             sources_, targets_, acc_, potentials_;
    DeviceArray<unsigned char> workspace_;
};
