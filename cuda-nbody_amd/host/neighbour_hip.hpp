// neighbour_hip.hpp -- NeighbourSurveyHIP<T>: nearest neighbours, counts within a radius, potentials and neighbour lists of states of N
// bodies through nb_neighbour_* (include/nbody_hip_neighbour.h, libnbody_hip_neighbour.so).  The outputs, the status record, the
// workspace and a staging copy of the positions are DeviceArrays (a device without room throws DeviceBadAlloc).  A refused call throws
// std::runtime_error carrying the nb_error_string name.  Calls are asynchronous on `stream`; the getters wait for the null stream.
#pragma once

#include "../../include/nbody_hip_neighbour.h"
#include "device_array.hpp"

#include <concepts>
#include <cstddef>
#include <cstdint>
#include <span>
#include <vector>

template <std::floating_point T> class NeighbourSurveyHIP {
 public:
    explicit NeighbourSurveyHIP(std::size_t num_bodies) : num_bodies_(num_bodies) {
        // the sizes the calls refuse are refused here, before anything is allocated
        hip_check(num_bodies <= 0xFFFFFFFFu ? nb_neighbour_workspace_bytes(static_cast<unsigned>(num_bodies), sizeof(T), &workspace_bytes_) : NB_ERR_INVALID_ARGUMENT,
                  "nb_neighbour_workspace_bytes");
        pos_        = DeviceArray<T>(4 * num_bodies);
        nearest_    = DeviceArray<unsigned>(num_bodies);
        nearest_d2_ = DeviceArray<T>(num_bodies);
        counts_     = DeviceArray<unsigned>(num_bodies);
        potentials_ = DeviceArray<T>(num_bodies);
        offsets_    = DeviceArray<unsigned long long>(num_bodies + 1);
        status_     = DeviceArray<nb_neighbour_status_t>(1);
        workspace_  = DeviceArray<unsigned char>(workspace_bytes_);
    }

    auto num_bodies() const noexcept { return num_bodies_; }

    // nearest neighbours, counts within radius_sq and (with_potentials) potentials of the device array `positions` (T[4 N], only read)
    auto survey(const T* positions, T radius_sq, T softening_sq, bool with_potentials, nb_stream_t stream = nullptr) -> void {
        const auto n = static_cast<unsigned>(num_bodies_);
        T* const   potentials = with_potentials ? potentials_.data() : nullptr;
        int        status;
        if constexpr (sizeof(T) == 4) {
            status = nb_neighbour_survey_f32(positions, n, radius_sq, nullptr, softening_sq, nearest_.data(), nearest_d2_.data(), counts_.data(), potentials, status_.data(),
                                             workspace_.data(), workspace_bytes_, stream);
        } else {
            status = nb_neighbour_survey_f64(positions, n, radius_sq, nullptr, softening_sq, nearest_.data(), nearest_d2_.data(), counts_.data(), potentials, status_.data(),
                                             workspace_.data(), workspace_bytes_, stream);
        }
        hip_check(status, "nb_neighbour_survey");
    }
    // ... of a state on the host
    auto survey(std::span<const T> positions, T radius_sq, T softening_sq, bool with_potentials) -> void {
        pos_.upload(positions);
        survey(pos_.data(), radius_sq, softening_sq, with_potentials);
    }

    // the neighbours within radius_sq as CSR lists of at most `capacity` entries in all; status().flags says whether they fitted
    auto lists(const T* positions, T radius_sq, std::size_t capacity, nb_stream_t stream = nullptr) -> void {
        if (indices_.size() < capacity) indices_ = DeviceArray<unsigned>(capacity);
        const auto n = static_cast<unsigned>(num_bodies_);
        int        status;
        if constexpr (sizeof(T) == 4) {
            status = nb_neighbour_lists_f32(positions, n, radius_sq, nullptr, offsets_.data(), capacity > 0 ? indices_.data() : nullptr, capacity, status_.data(), workspace_.data(),
                                            workspace_bytes_, stream);
        } else {
            status = nb_neighbour_lists_f64(positions, n, radius_sq, nullptr, offsets_.data(), capacity > 0 ? indices_.data() : nullptr, capacity, status_.data(), workspace_.data(),
                                            workspace_bytes_, stream);
        }
        hip_check(status, "nb_neighbour_lists");
    }

    auto status() const -> nb_neighbour_status_t {
        nb_neighbour_status_t out{};
        status_.download(std::span<nb_neighbour_status_t>(&out, 1));
        return out;
    }
    auto get_nearest_index(std::span<unsigned> out) const -> void { nearest_.download(out); }
    auto get_nearest_dist_sq(std::span<T> out) const -> void { nearest_d2_.download(out); }
    auto get_counts(std::span<unsigned> out) const -> void { counts_.download(out); }
    auto get_potentials(std::span<T> out) const -> void { potentials_.download(out); }
    auto get_offsets(std::span<unsigned long long> out) const -> void { offsets_.download(out); }
    auto get_indices(std::span<unsigned> out) const -> void { indices_.download(out); }

 private:
    std::size_t                        num_bodies_;
    std::size_t                        workspace_bytes_ = 0;
    DeviceArray<T>                     pos_, nearest_d2_, potentials_;
    DeviceArray<unsigned>              nearest_, counts_, indices_;
    DeviceArray<unsigned long long>    offsets_;
    DeviceArray<nb_neighbour_status_t> status_;
    DeviceArray<unsigned char>         workspace_;
};
