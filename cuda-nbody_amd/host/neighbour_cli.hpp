// neighbour_cli.hpp -- `nbody --neighbours=<radius>`: after a run, the closest pair, the neighbour counts within the radius and the
// deepest potential of the final state (NeighbourSurveyHIP, libnbody_hip_neighbour.so).
#pragma once

#include <span>

// Prints three lines:
//   closest pair: bodies I and J, separation S
//   neighbours within R: mean M, largest C at body B
//   deepest potential: P at body B                      (softened as the run: -sum m_j / sqrt(d^2 + softening_sq))
auto report_neighbours(std::span<const float> positions, double radius, float softening_sq) -> void;
auto report_neighbours(std::span<const double> positions, double radius, double softening_sq) -> void;
