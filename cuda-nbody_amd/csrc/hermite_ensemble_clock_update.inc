// hermite_ensemble_clock_update.inc -- what the clock kernel of an ensemble does with ONE system once its next dt can be formed, as text
// inside hermite_ensemble_clock (hermite_ensemble.hip) and hermite6_ensemble_clock (hermite6_ensemble.hip), which differ only in next_dt().
// The kernel has defined T, the system s, next_dt() (the scheme's own expression of the system's partial minima), dt_out, clocks, begin, src
// and the system's tally t (hermite_ensemble_clock.inc).
//   dt_out != nullptr   dt_out[s] = dt                                     (*_ensemble_timestep_*)
//   begin               the clock of a run that starts                      (*_ensemble_begin_*)
//   else                the clock after this call's step, by the rule of the header (*_ensemble_advance_*), and the system's tally
        if (dt_out != nullptr) {
            dt_out[s] = next_dt();
        } else if (begin) {
            const T       dt = next_dt();
            EnsembleClock c{0.0, static_cast<double>(dt), 0.0, 0u, dt > T(0) ? 0u : kClockStalled};
            clocks[s] = c;
        } else {
            EnsembleClock c = clocks[s];
            T             dt;
            const int     what = clock_decision<T>(c, src.t_stop, src.dt_max, dt);
            if (what == kFinish) {
                c.flags |= kClockDone, c.time = src.t_stop;
                clocks[s] = c;
            } else if (what >= kStep) {
                c.time    = what == kLastStep ? src.t_stop : c.time + static_cast<double>(dt);
                c.dt_last = static_cast<double>(dt);
                c.steps += 1;
                c.dt_next = static_cast<double>(next_dt());
                if (what == kLastStep) c.flags |= kClockDone;
                if (!(c.dt_next > 0) && !(c.flags & kClockDone)) c.flags |= kClockStalled;
                clocks[s]     = c;
                t.stepped     = 1;
                t.min_dt_last = c.dt_last;
            }
            t.systems = 1, t.done = (c.flags & kClockDone) ? 1 : 0, t.stalled = (c.flags & kClockStalled) ? 1 : 0, t.total_steps = c.steps, t.min_time = c.time;
        }
