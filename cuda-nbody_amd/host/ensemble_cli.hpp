// ensemble_cli.hpp -- `nbody --systems=<B>`: B independent systems of --numbodies bodies stepped in one launch (BodyEnsembleHIP), or, with
// --integrator=hermite-ensemble, by 4th-order Hermite steps with one dt for all or a time step per system (BodyEnsembleHIPHermite), or,
// with --integrator=hermite6-ensemble, by 6th-order Hermite steps in the same two forms (BodyEnsembleHIPHermite6), or,
// with --integrator=hermite-block-ensemble, by block time steps, a step per BODY (BodyEnsembleHIPHermiteBlock), or,
// with --integrator=hermite6-block-ensemble, by 6th-order block time steps (BodyEnsembleHIPHermite6Block).
#pragma once

#include "nbody_types.hpp"

#include <cstddef>
#include <filesystem>

struct EnsembleRun {
    bool                  fp64 = false;
    std::size_t           num_bodies = 0, num_systems = 0;
    int                   mode = 0;
    NBodyConfig           config = NBodyConfig::NBODY_CONFIG_SHELL;
    NBodyParams           params{};         // the demo row every system runs (dt, damping, softening)
    bool                  benchmark = false;
    int                   iterations = 10;
    std::size_t           steps = 0;
    std::filesystem::path dump;
    bool                  hermite = false;  // --integrator=hermite-ensemble or hermite6-ensemble
    bool                  sixth = false;    // --integrator=hermite6-ensemble (`hermite` is set too) or hermite6-block-ensemble (`block` is): that run, with the 6th-order scheme
    double                t_end = 0.0;      // hermite: > 0 runs the adaptive form to this time (--t-end), else --steps fixed steps of params.time_step
    double                eta = 0.02;       // hermite, adaptive: the accuracy parameter of the systems' time steps (--eta); block: of the bodies'
    bool                  block = false;    // --integrator=hermite-block-ensemble or hermite6-block-ensemble: dt_max = params.time_step; --t-end, or --steps=K intervals of dt_max
    int                   levels = 30;      // block: the deepest level (--levels)
    bool                  energies = false; // --energies: every system's energy at the start and at the end (EnsembleEnergyHIP), two lines
};

// Starts from the current rand() state (main has applied --seed): system 0 is the single-system start-up state (the same three
// randomise_bodies segments), systems 1 .. B-1 the next B-1 draws of the active precision with the same scales.
auto run_ensemble(const EnsembleRun& run) -> void;
