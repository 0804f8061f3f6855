// The body of ONE sub-step of one env's cars: integrator, collisions, progress / lap / reward / done.  Program text that is
// included where it runs, not a function: rc_dynamics_kernel's dynamics_env includes it in its action-repeat loop (so its code is
// what it was before the look-ahead existed, byte for byte - as a function the same body was simplified on its own before it
// was inlined, and the dynamics kernels came out with other schedules: A = 1 168 -> 190 VGPRs, 1 - 5 % slower), and
// dynamics_substep (racecar_step.h) includes it for the look-ahead.  One text, two instantiations.
// Expects in scope: template values A, DR; p (RcParams), t (RcTrackDev), car[A], motor[A], steer[A], vp[A][RC_VP_COUNT] (read only
// where DR), steps (int, counted here), and the macro RC_NSTEP_SLOT(a, k) = the address of slot k of car slot a's n_step_progress
// window.  Leaves `bool stop`: the env finished on this sub-step.
            // --- kinematic bicycle, explicit Euler (H2)
#pragma unroll
            for (int a = 0; a < A; ++a) {
                Car &c = car[a];
                const float m = motor[a];
                const float accel_max = DR ? vp[a][RC_VP_ACCEL_MAX] : RCS_ACCEL_MAX, drag = DR ? vp[a][RC_VP_DRAG] : RCS_DRAG;
                const float max_vel = DR ? vp[a][RC_VP_MAX_VEL] : RCS_MAX_VEL, steer_step = DR ? vp[a][RC_VP_STEER_STEP] : RCS_STEER_STEP;
                const float steer_gain = DR ? -vp[a][RC_VP_WHEEL_MAX] : RCS_STEER_GAIN;
                const float force = fabsf(m) * accel_max;
                const float acc = (m >= 0.0f ? force : -force) - drag * c.v;
                c.v = clampf(c.v + acc * RCS_DT, 0.0f, max_vel);
                const float dd = clampf(steer[a] * steer_gain - c.dl, -steer_step, steer_step);
                c.dl = c.dl + dd;
                float sd, cd;
                sincos32(c.dl, sd, cd);
                c.om = (c.v / RCS_WHEELBASE) * (sd / cd);
                c.x = c.x + (c.v * c.ct) * RCS_DT;
                c.y = c.y + (c.v * c.st) * RCS_DT;
                float th = c.th + c.om * RCS_DT;
                th = th > RCS_PI ? th - RCS_TWO_PI : th;
                th = th < -RCS_PI ? th + RCS_TWO_PI : th;
                c.th = th;
                sincos32(th, c.st, c.ct);
                c.ac = acc;
            }
            steps += 1;
            // --- collisions (H5)
#pragma unroll
            for (int a = 0; a < A; ++a) {
                car[a].wall = wall_hit(t, car[a]);
                car[a].opp = 0;
            }
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int b = a + 1; b < A; ++b) {
                    const int o = obb_overlap(car[a], car[b]);
                    car[a].opp |= o;
                    car[b].opp |= o;
                }
            // --- progress, lap, reward, done (H4, H15)
            const float time = (float)steps * RCS_DT;
            bool stop = false;
#pragma unroll
            for (int a = 0; a < A; ++a) {
                Car &c = car[a];
                float p_new = progress_at(t, c.x, c.y);
                const float p_old = c.pr;
                const int lap_old = c.lap, cp_old = c.cp;
                p_new = p_new >= 0.0f ? p_new : p_old;
                int cp_new = (int)(p_new * (float)RCS_N_CHECKPOINTS);
                cp_new = cp_new < RCS_N_CHECKPOINTS - 1 ? cp_new : RCS_N_CHECKPOINTS - 1;
                int d = cp_new - cp_old;
                d = d < 0 ? d + RCS_N_CHECKPOINTS : d;
                const bool fwd = d > 0 && d <= RCS_N_CHECKPOINTS / 2;
                const bool bwd = d > RCS_N_CHECKPOINTS / 2;
                const int lap = lap_old + ((fwd && cp_new < cp_old) ? 1 : 0) - ((bwd && cp_new > cp_old) ? 1 : 0);
                c.wrong = fwd ? 0 : (bwd ? 1 : c.wrong);
                c.cp = (fwd || bwd) ? cp_new : cp_old;
                c.lap = lap;
                c.pr = p_new;
                const bool collided = (c.wall | c.opp) != 0;
                float r;
                bool done;
                const int task = p.car_task[a];
                if (task == 2) {
                    // n_step_progress, the secondary agents' task of baselines/scenarios/max_progress/columbia.yml:17-18:
                    // total progress gained over the last n_steps sub-steps, no collision term, never done
                    float *h = RC_NSTEP_SLOT(a, steps % p.n_steps);
                    const float total = (float)(lap - 1) + p_new;
                    r = (total - *h) * RCS_PROGRESS_REWARD;
                    *h = total;
                    done = false;
                } else if (task == 0) {
                    const float delta = (float)(lap - lap_old) + (p_new - p_old);
                    r = delta * RCS_PROGRESS_REWARD + (collided ? p.collision_reward : 0.0f);
                    done = (collided && p.terminate_on_collision) || lap > p.laps || time > p.time_limit;
                } else {   // baselines/racing/environment/tasks.py:6-18
                    r = c.wall ? -1.0f : -rcd::exp32(fabsf(steer[a]) - c.v);
                    done = false;
                }
                c.rew = c.rew + r;
                c.done = done ? 1 : 0;
                stop |= done;
            }
