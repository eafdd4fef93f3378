/*
 * mpcbatch_multi.h — the multi-start entries of libmpcbatch's C ABI.  Included by mpcbatch.h (include that one): this file needs its
 * types and constants and stands inside its extern "C" block.
 */
#ifndef MPCBATCH_MULTI_H
#define MPCBATCH_MULTI_H
#ifndef MPCBATCH_H
#error "include mpcbatch.h, which includes this file"
#endif

/* ---- multi-start solve: K starts per instance, the best solution kept on the device ------------------------------------------------
 * The kernels find a local minimum, and which one depends on the start (passing an obstacle on the left or on the right is a discrete
 * choice).  These entries solve every instance from K starts in ONE launch of K * B instances and keep, per instance, the cheapest
 * solution found; nothing but the winner has to leave the device.
 *   controls [K, 2]  HOST array (in both entries) of (steer, accel).  Candidate k of instance b starts from the row whose U part is that
 *                    pair at every stage and whose X part is x0[b] at every node (cfg.init_rollout = 1: the solve rolls X out itself).
 *   z0 [B, nz]       NULL, or the caller's start of candidate 0, used verbatim (controls[0] is then ignored): the warm start of a closed
 *                    loop plus K - 1 alternatives.  controls may be NULL only for K = 1 with z0.
 *                    Every candidate is a solve WITH a start vector: cfg.start_steer does not act and cfg.second_start = 3 behaves as 2,
 *                    exactly as mpcb_solve_device(z0 != NULL).  K = 1 with z0 is mpcb_solve_device with that z0, bit for bit.
 *   expanded batch   instance e = b * K + k; x0, xs and the obstacle rows (either obs_kind) of b are replicated K times into a workspace
 *                    the handle owns (it grows on demand and is freed in mpcb_destroy), then one ordinary solve of K * B instances runs:
 *                    everything the handle accepts (either model, a time grid, RK4, general gamma, up to 8 obstacles) works.
 *   selection        a candidate is eligible when its status is MPCB_ST_SOLVED or MPCB_ST_ACCEPTABLE and its objective is finite.
 *                    Walking k = 0..K-1 the first eligible candidate is the incumbent; a later one replaces it only if
 *                    obj_k < obj_inc - obj_margin * max(1, |obj_inc|).  No eligible candidate: candidate 0, with its failure status.
 *   outputs          z, obj, status, iters, kkt, lam_g, lam_x: the winner's, as mpcb_solve returns them (each may be NULL except z);
 *                    which [B] the winner's index; n_ok [B] the number of eligible candidates; n_basins [B] the number of distinct
 *                    solutions: walking the eligible candidates in index order, one is a new representative when
 *                    max_i |z_k[i] - z_r[i]| > basin_tol for every earlier representative r (int32, each may be NULL);
 *                    z_all [B, K, nz], obj_all / status_all / iters_all [B, K]: every candidate's result (each may be NULL; where given,
 *                    the solve writes there directly).
 * Refused before anything is launched, outputs untouched: K outside 1..MPCB_MULTI_MAX, B < 0, K * B beyond INT32_MAX, a non-finite
 * entry of controls, controls NULL (unless K = 1 with z0), z NULL, x0 / xs NULL, obs NULL with n_obs > 0, a negative or non-finite
 * obj_margin / basin_tol (MPCB_E_INVALID); a device group (MPCB_E_UNSUPPORTED).  B = 0 returns MPCB_OK.
 * mpcb_solve_multi takes host pointers; mpcb_solve_multi_device device pointers (asynchronous unless sync != 0).  Both wait for the
 * launch lanes and run on the handle's own stream; results do not depend on mpcb_set_inflight.  There is no per-stage reference and no
 * parameter set in these calls. */
#define MPCB_MULTI_MAX 8
int mpcb_solve_multi(mpcb_handle* h, int32_t B, int32_t K,
                     const double* x0, const double* xs, const double* obs, int32_t obs_kind, const double* z0,
                     const double* controls, double obj_margin, double basin_tol,
                     double* z, double* obj, int32_t* status, int32_t* iters, double* kkt, double* lam_g, double* lam_x,
                     int32_t* which, int32_t* n_ok, int32_t* n_basins,
                     double* z_all, double* obj_all, int32_t* status_all, int32_t* iters_all);
int mpcb_solve_multi_device(mpcb_handle* h, int32_t B, int32_t K,
                            const double* d_x0, const double* d_xs, const double* d_obs, int32_t obs_kind, const double* d_z0,
                            const double* controls, double obj_margin, double basin_tol,
                            double* d_z, double* d_obj, int32_t* d_status, int32_t* d_iters, double* d_kkt, double* d_lam_g, double* d_lam_x,
                            int32_t* d_which, int32_t* d_n_ok, int32_t* d_n_basins,
                            double* d_z_all, double* d_obj_all, int32_t* d_status_all, int32_t* d_iters_all, int32_t sync);

#endif /* MPCBATCH_MULTI_H */
