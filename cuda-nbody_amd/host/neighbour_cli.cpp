// neighbour_cli.cpp -- `nbody --neighbours=<radius>` (neighbour_cli.hpp)
#include "neighbour_cli.hpp"

#include "neighbour_hip.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

template <typename T> auto report(std::span<const T> positions, double radius, T softening_sq) -> void {
    const auto n         = positions.size() / 4;
    const T    radius_sq = static_cast<T>(radius) * static_cast<T>(radius);
    auto       survey    = NeighbourSurveyHIP<T>(n);
    survey.survey(positions, radius_sq, softening_sq, true);
    const auto     status = survey.status();
    std::vector<T> potentials(n);
    survey.get_potentials(potentials);
    if (status.closest_i == NB_NEIGHBOUR_NONE) {
        std::printf("closest pair: none\n");
    } else {
        std::printf("closest pair: bodies %u and %u, separation %.9g\n", status.closest_i, status.closest_j, std::sqrt(status.closest_dist_sq));
    }
    std::printf("neighbours within %.9g: mean %.9g, largest %u at body %u\n", radius, static_cast<double>(status.total_neighbours) / static_cast<double>(n), status.max_count,
                status.max_count_body);
    const auto deepest = std::min_element(potentials.begin(), potentials.end());  // (the lowest body of equal values)
    std::printf("deepest potential: %.9g at body %zu\n", static_cast<double>(*deepest), static_cast<std::size_t>(deepest - potentials.begin()));
}

}  // namespace

auto report_neighbours(std::span<const float> positions, double radius, float softening_sq) -> void { report<float>(positions, radius, softening_sq); }
auto report_neighbours(std::span<const double> positions, double radius, double softening_sq) -> void { report<double>(positions, radius, softening_sq); }
