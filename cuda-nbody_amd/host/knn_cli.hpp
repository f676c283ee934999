// knn_cli.hpp -- `nbody --knn=<K>`: after a run, the density centre, the density and core radii, the densest body, the K-th-neighbour
// distances and the Lagrangian radii of the final state (KnnSurveyHIP, libnbody_hip_knn.so; the Lagrangian radii from a host sort).
#pragma once

#include <array>
#include <span>
#include <vector>

// Prints five lines (every number with 17 significant digits: the record's bits):
//   density centre: X Y Z (K = k, D bodies defined, G degenerate)          or   density centre: none (...)   when no body has a density
//   density radius: R, core radius: C
//   densest body: B, density RHO
//   K-th neighbour distance: smallest A, largest B
//   Lagrangian radii (10%, 50%, 90%): A B C                                  (about the density centre; left out when there is none)
auto report_knn(std::span<const float> positions, unsigned k) -> void;
auto report_knn(std::span<const double> positions, unsigned k) -> void;

// For each fraction f the smallest distance from `centre` whose bodies (all within it; distances in double) hold at least f times the total mass.
// positions: T[4 N] = {x, y, z, mass}
auto lagrangian_radii(std::span<const float> positions, const std::array<double, 3>& centre, std::span<const double> fractions) -> std::vector<double>;
auto lagrangian_radii(std::span<const double> positions, const std::array<double, 3>& centre, std::span<const double> fractions) -> std::vector<double>;
