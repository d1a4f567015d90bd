/*
 * pyqsm_hip.h — C-ABI of libpyqsm_hip.so, the MI355X (gfx950) implementation of
 * pyQSM's point-cloud geometry hot path.
 *
 * The reference (wischmcj/pyQSM) is pure Python and has no FFI of its own; the
 * seam it offers is a handful of Python call sites into third-party engines.
 * Every entry point below names the reference call it stands in for
 * (file:line relative to the reference root).  The Python wrappers in
 * pyqsm_amd/ bind these symbols with ctypes and expose the reference's own
 * function names and signatures on top.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every buffer it passes in;
 *     arrays are C-contiguous; no exceptions cross the ABI
 *   - return 0 on success, a negative PYQSM_E* code on failure; the message is
 *     available (per thread) from pyqsm_last_error()
 *   - "host" entry points take host pointers and stage through HBM themselves;
 *     "_dev" entry points take device pointers (HBM-resident input/output,
 *     obtained from pyqsm_dev_malloc or any hipMalloc'd allocation) and are
 *     asynchronous on the library's per-device stream until pyqsm_sync()
 *   - the library owns one HIP stream and one scratch arena per device and
 *     calling thread: threads may call concurrently, each is ordered on its own
 *     stream (pyqsm_stream / pyqsm_sync / pyqsm_prof_* act on the caller's)
 */
#ifndef PYQSM_HIP_H
#define PYQSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYQSM_OK 0
#define PYQSM_EINVAL (-1)   /* bad argument (null pointer, negative size, ...)   */
#define PYQSM_EHIP (-2)     /* a HIP runtime call failed                         */
#define PYQSM_ENODEV (-3)   /* no usable GPU / device index out of range         */
#define PYQSM_ERANGE (-4)   /* input outside what the kernels are built for      */
#define PYQSM_ENOMEM (-5)   /* device or host allocation failed                  */
#define PYQSM_ENOCONV (-6)  /* CG stopped (max_it / stagnation) above rtol; best
                               iterate is still returned                         */

#define PYQSM_MISS_PRIM 0xFFFFFFFFu /* primitive id reported for a ray that hits nothing */

/* ---- library / device management ------------------------------------- */

/* Number of visible GPUs (0 when none); never fails. */
int pyqsm_device_count(void);
/* Create the calling thread's context for `device` (stream + arena). Idempotent. */
int pyqsm_init(int device);
/* Destroy every context created by pyqsm_init. */
int pyqsm_shutdown(void);
/* Message of the last failure on the calling thread ("" when none). */
const char* pyqsm_last_error(void);
/* "pyqsm_hip <version> gfx950" */
const char* pyqsm_version(void);
/* Block until the library stream of `device` has drained. */
int pyqsm_sync(int device);
/* The library's hipStream_t for `device`, as an opaque pointer (for callers
 * that order their own work against it). */
void* pyqsm_stream(int device);

/* HBM buffers for the _dev entry points. */
int pyqsm_dev_malloc(int device, size_t bytes, void** out);
int pyqsm_dev_free(int device, void* p);
int pyqsm_h2d(int device, void* dst_dev, const void* src_host, size_t bytes);
int pyqsm_d2h(int device, void* dst_host, const void* src_dev, size_t bytes);
/* Release memory returned through an `**` out-parameter of a host entry point. */
void pyqsm_free(void* p);
/* A host buffer from the same pool those out-parameters come from: page-locked when it is a
 * megabyte or more (plain malloc otherwise or when page-locking fails), released with pyqsm_free.
 * Results written into such a buffer leave the device at link speed and without blocking the
 * caller's thread; into pageable memory every 24 MB of pyqsm_extract_skeleton's per-step shifts
 * cost 12 ms of staging (0.26 s of a 2.8 s loop). NULL when out of memory. */
void* pyqsm_host_alloc(size_t bytes);

/* HIP-event timers around named kernel groups on the library stream.
 * Disabled by default (zero overhead); bench.py switches them on to measure
 * the dominant kernel's average launch duration live. on = 1: phase timers and the
 * dominant kernels of each path; on = 2: also single kernels inside the solver's
 * iteration loops (k_bspmv_f, k_down_l0, k_up_l0: adds two event records per launch)
 * and the counters of the DBSCAN core pass ("core_pair_tests": launches =
 * lane-tests executed, ms = 0; "core_band_lanes": launches = points the fp32 decision
 * left to the fp64 pass that had a distance in the band around eps^2, ms = 0). */
int pyqsm_prof_enable(int device, int on);
int pyqsm_prof_reset(int device);
/* Sum of elapsed ms and number of launches recorded under `name`
 * since the last reset. Synchronises the stream. */
int pyqsm_prof_get(int device, const char* name, double* total_ms, int64_t* launches);

/* ---- ray x triangle sweep -------------------------------------------- */
/*
 * Closest-hit ray casting against a triangle soup, brute force (no BVH).
 * Stands in for open3d.t.geometry.RaycastingScene.add_triangles + cast_rays as
 * called at pyQSM/viz/ray_casting.py:275-279 (also :218-225, :316-319).
 *   verts  f32 [V,3]     tris  i32 [T,3] (indices into verts)
 *   rays   f32 [R,6] = (ox,oy,oz,dx,dy,dz); d need not be unit, t is in units of |d|
 *   t_hit  f32 [R]  (+inf on miss)      prim_id u32 [R] (PYQSM_MISS_PRIM on miss)
 *   uv     f32 [R,2] or NULL; hit = (1-u-v)*v0 + u*v1 + v*v2 (ray_casting.py:172-180)
 *   Ties in t go to the lowest triangle index. A hit needs t > 0.
 */
int pyqsm_cast_rays(const float* verts, int64_t V, const int32_t* tris, int64_t T,
                    const float* rays, int64_t R,
                    float* t_hit, uint32_t* prim_id, float* uv, int32_t device);

/* Device-resident form. `tri9` is the expanded mesh produced by
 * pyqsm_expand_tris_dev: f32 [T,12] = (v0.xyz, e1.xyz, e2.xyz, 0,0,0). */
int pyqsm_expand_tris_dev(const float* verts_dev, int64_t V, const int32_t* tris_dev,
                          int64_t T, float* tri12_dev, int32_t device);
int pyqsm_cast_rays_dev(const float* tri12_dev, int64_t T, const float* rays_dev, int64_t R,
                        float* t_hit_dev, uint32_t* prim_id_dev, float* uv_dev,
                        int32_t device);

/* All intersections (RaycastingScene.list_intersections, ray_casting.py:168) and
 * crossing counts (compute_occupancy, ray_casting.py:65-69 = odd count).
 *   counts i32 [R] = number of triangles each ray crosses with t > 0.
 *   If hits_cap > 0: up to hits_cap records (ray_id u32, prim_id u32, t f32, u f32, v f32)
 *   are written, ordered by ray id then triangle id; *n_hits = total found. */
int pyqsm_list_intersections(const float* verts, int64_t V, const int32_t* tris, int64_t T,
                             const float* rays, int64_t R, int32_t* counts,
                             uint32_t* ray_ids, uint32_t* prim_ids, float* t, float* uv,
                             int64_t hits_cap, int64_t* n_hits, int32_t device);

/*
 * Unsigned distance from query points to the mesh and the index of the closest
 * triangle — open3d RaycastingScene.compute_distance, which `mri`
 * (pyQSM/viz/ray_casting.py:237-260) reaches through compute_signed_distance; the sign
 * is the occupancy of pyqsm_list_intersections (inside = negative), applied by the
 * wrapper. Brute force, fp32; lowest triangle index on ties; T = 0 gives +inf.
 *   qry f32 [Q,3]; dist f32 [Q]; prim u32 [Q].
 */
int pyqsm_point_mesh_distance(const float* verts, int64_t V, const int32_t* tris, int64_t T,
                              const float* qry, int64_t Q, float* dist, uint32_t* prim,
                              int32_t device);

/* ---- the ray sweep over several GPUs (RCCL over xGMI) ------------------ */
/*
 * One process driving n_devices GPUs of the node (stands in for
 * scene.cast_rays(rays) at pyQSM/viz/ray_casting.py:275-279 on more than one GPU):
 * the mesh is expanded on device 0 and replicated with ncclBroadcast, rays are split
 * into contiguous shards (sizes differ by at most one, in device order), every device
 * sweeps its shard, and ncclAllGather leaves the full (t, prim[, uv]) on every device;
 * device 0's copy goes to the host arrays. Results are identical to pyqsm_cast_rays
 * (rays are independent). Same argument meaning as pyqsm_cast_rays; n_devices <= 0
 * means every visible GPU; n_devices = 1 still goes through RCCL.
 */
int pyqsm_cast_rays_multi(const float* verts, int64_t V, const int32_t* tris, int64_t T,
                          const float* rays, int64_t R,
                          float* t_hit, uint32_t* prim_id, float* uv, int32_t n_devices);

/* The contiguous shard [*begin, *end) of `rank` among `world` ranks over n items, as
 * pyqsm_cast_rays_multi splits the rays (sizes differ by at most one, in rank order; needs no GPU). */
int pyqsm_shard_bounds(int64_t n, int32_t world, int32_t rank, int64_t* begin, int64_t* end);

/*
 * One process PER GPU (torchrun-style launches): a communicator per process and the
 * data-path collectives on the library stream of the rank's device. Rank 0 creates the
 * id and ships its PYQSM_COMM_ID_BYTES bytes to the other ranks by any means (a file, a
 * socket, a CPU rendezvous); pyqsm_comm_init_rank is collective. The _dev calls take
 * device pointers and are asynchronous until pyqsm_sync(device).
 *   broadcast: in place, `bytes` from rank `root`;  all_gather: recv holds world *
 *   bytes_per_rank, rank r's block at offset r * bytes_per_rank (send may alias its
 *   own block);  all_reduce_max: host scalar in/out, returns when every rank has the
 *   maximum (doubles as a barrier).
 */
#define PYQSM_COMM_ID_BYTES 128
int pyqsm_comm_unique_id(uint8_t* id);
int pyqsm_comm_init_rank(const uint8_t* id, int32_t world, int32_t rank, int32_t device);
int pyqsm_comm_finalize(void);
/* world = 0 when no communicator exists */
int pyqsm_comm_info(int32_t* world, int32_t* rank, int32_t* device);
int pyqsm_comm_broadcast_dev(void* buf_dev, int64_t bytes, int32_t root);
int pyqsm_comm_all_gather_dev(const void* send_dev, void* recv_dev, int64_t bytes_per_rank);
int pyqsm_comm_all_reduce_max(double* value);

/* ---- eps-neighbourhood clustering (DBSCAN) ---------------------------- */
/*
 * Stands in for sklearn.cluster.DBSCAN(eps, min_samples).fit(points) at
 * pyQSM/math_utils/fit.py:223 and open3d PointCloud.cluster_dbscan at
 * pyQSM/geometry/point_cloud_processing.py:185,209.
 *   xyz f64 [n,3]; labels i64 [n] (-1 = noise); is_core u8 [n] (may be NULL)
 * Semantics (bit-exact with scikit-learn): core <=> #{j : d2(i,j) <= eps*eps} >=
 * min_pts counting i itself, d2 = ((dx*dx + dy*dy) + dz*dz) in fp64 without
 * contraction; clusters = connected components of the core-core eps graph,
 * numbered by ascending smallest core index; a border point takes the smallest
 * cluster label among its core neighbours.
 */
int pyqsm_dbscan(const double* xyz, int64_t n, double eps, int32_t min_pts,
                 int64_t* labels, uint8_t* is_core, int32_t device);
int pyqsm_dbscan_dev(const double* xyz_dev, int64_t n, double eps, int32_t min_pts,
                     int64_t* labels_dev, uint8_t* is_core_dev, int64_t* n_clusters,
                     int32_t device);
/*
 * The same with the neighbourhood's boundary as a parameter. radius_inclusive != 0:
 * d2 <= eps*eps, scikit-learn's (the two calls above). radius_inclusive == 0: d2 < eps*eps —
 * what open3d cluster_dbscan (pyQSM/geometry/point_cloud_processing.py:185,209) computes if
 * nanoflann's radius search compares strictly (Open3D is not installable
 * here, so which of the two it is stays unpinned: this is the switch for whoever can check).
 * Everything else — self counted, numbering, border rule — is unchanged.
 */
int pyqsm_dbscan_ex(const double* xyz, int64_t n, double eps, int32_t min_pts,
                    int32_t radius_inclusive, int64_t* labels, uint8_t* is_core, int32_t device);
int pyqsm_dbscan_dev_ex(const double* xyz_dev, int64_t n, double eps, int32_t min_pts,
                        int32_t radius_inclusive, int64_t* labels_dev, uint8_t* is_core_dev,
                        int64_t* n_clusters, int32_t device);
/*
 * A read-out of the cell directory DBSCAN bins with, for tests: plans and bins the cloud exactly as
 * pyqsm_dbscan does (first call on a context: planned on the host; a repeat: the device plan;
 * PYQSM_DBSCAN_PLAN, PYQSM_COORD_F32 and PYQSM_DBSCAN_BIN are honoured), then evaluates the
 * directory on the device. dims_out i32 [3]: the grid's cells per axis, borders included;
 * begin_out i32 [ncell + 1], ncell = the product of the dims: begin_out[c] = number of points in
 * cells with id < c. PYQSM_ERANGE when ncell + 1 > cap (the entries begin_out has room for; the
 * dims are not written then).
 */
int pyqsm_octant_directory(const double* xyz, int64_t n, double eps, int32_t* dims_out,
                           int32_t* begin_out, int64_t cap, int32_t device);
/*
 * The core pass over fp32 records counts neighbours with two clamped fp32 ramps of the squared distance d,
 * s_in = sat(A - K d) and s_hi = sat(B - K d) (one fma each): s_in > 0 only where d <= lo, s_hi = 1
 * wherever d <= hi, lo and hi the fp32 thresholds below and above which fp32 decides a pair as fp64 would.
 * For tests:
 * pyqsm_core_ramp_constants needs no GPU. out f32 [6]: lo, hi, K, A, B as pyqsm_dbscan_ex derives them
 *   from eps and the radius rule, and 1 or 0: whether the ramp form runs at this eps (0: the fp64
 *   kernel does; K, A, B may then be 0).
 * pyqsm_core_ramp_probe evaluates the ramps on the device, with the function the core pass calls.
 *   d f32 [n] (host), s_in_out and s_hi_out f32 [n] (host). PYQSM_EINVAL where the ramp form does not run.
 */
int pyqsm_core_ramp_constants(double eps, int32_t radius_inclusive, float* out);
int pyqsm_core_ramp_probe(const float* d, int64_t n, double eps, int32_t radius_inclusive,
                          float* s_in_out, float* s_hi_out, int32_t device);

/* ---- k nearest neighbours --------------------------------------------- */
/*
 * Exact kNN over one cloud (query set = data set). Stands in for the neighbour
 * search inside robust_laplacian.point_cloud_laplacian (pyQSM/geometry/
 * skeletonize.py:253-255) and scipy cKDTree.query (pyQSM/geometry/
 * reconstruction.py:238-240).
 *   idx i32 [n,k], d2 f64 [n,k] (squared distance), ascending by (d2, index);
 *   exclude_self != 0 drops the query point itself. Rows are padded with
 *   idx = n, d2 = +inf when the cloud has fewer than k (other) points.
 */
int pyqsm_knn(const double* xyz, int64_t n, int32_t k, int32_t exclude_self,
              int32_t* idx, double* d2, int32_t device);
int pyqsm_knn_dev(const double* xyz_dev, int64_t n, int32_t k, int32_t exclude_self,
                  int32_t* idx_dev, double* d2_dev, int32_t device);

/* ---- RANSAC circle / cylinder ------------------------------------------ */
/*
 * Stands in for pyransac3d.Circle().fit / Cylinder().fit as called at
 * pyQSM/math_utils/fit.py:277-283. The caller supplies the 3-point samples
 * (the reference draws them from Python's unseeded `random`), one row per
 * hypothesis, so that runs are reproducible.
 *   pts f64 [n,3]; triples i64 [H,3]; shape 0 = circle, 1 = cylinder
 *   center[3], axis[3], *radius: model of the winning hypothesis (first
 *   hypothesis with a strictly larger inlier count wins)
 *   inliers i64 [n] capacity, ascending; *n_inliers = count; *best = winning row
 *   (-1 and n_inliers = 0 when no hypothesis has an inlier; center, axis and radius
 *   are then left as they were).
 * One call is a batch of one set (pyqsm_ransac_batch below) and has its limit: more
 * than 65535 tiles of 1024 points (n > 67 107 840) is refused with PYQSM_ERANGE and a
 * message before anything is copied, as in the batch, the count and the plane calls.
 */
int pyqsm_ransac(const double* pts, int64_t n, const int64_t* triples, int64_t H,
                 int32_t shape, double thresh, double center[3], double axis[3],
                 double* radius, int64_t* inliers, int64_t* n_inliers, int64_t* best,
                 int32_t device);
/* The two halves separately: models f64 [H,8] = (cx,cy,cz, ax,ay,az, r, valid). */
int pyqsm_ransac_models(const double* pts, int64_t n, const int64_t* triples, int64_t H,
                        double* models, int32_t device);
int pyqsm_ransac_count(const double* pts, int64_t n, const double* models, int64_t H,
                       int32_t shape, double thresh, int32_t* counts, int32_t device);
/*
 * Many independent fits in one call — the z-slices of a stem, each fitted like
 * pyQSM/math_utils/fit.py:277-283 fits one cluster (a call per slice is 0.6 ms of
 * launches and round trips for 0.05 ms of work). S point sets stacked in pts
 * (seg_start i64 [S+1], from 0 to n), H hypotheses per set: triples i64 [S,H,3]
 * with indices LOCAL to the set (a set with fewer than three points gets rows of -1).
 * Per set what pyqsm_ransac returns: centers f64 [S,3], axes f64 [S,3], radii f64 [S],
 * best i64 [S] (-1: no hypothesis with an inlier), n_inliers i64 [S], and the inliers
 * as ascending local indices, set after set, in inliers i64 [n] (capacity).
 */
int pyqsm_ransac_batch(const double* pts, int64_t n, const int64_t* seg_start, int64_t n_seg,
                       const int64_t* triples, int64_t H, int32_t shape, double thresh,
                       double* centers, double* axes, double* radii, int64_t* inliers,
                       int64_t* n_inliers, int64_t* best, int32_t device);

/* ---- plane segmentation -------------------------------------------------- */
/*
 * Stands in for Open3D's PointCloud.segment_plane, which the reference calls at
 * pyQSM/geometry/point_cloud_processing.py:182-183 (recollected from Open3D, parity
 * unpinned; tests/plane_restatement.py states this contract).
 * A plane is (a, b, c, d) with a unit normal whose sign makes c > 0, or c == 0 and
 * b > 0, or c == b == 0 and a > 0. A hypothesis comes from m sampled points, 3 <= m <= 32:
 * the plane through them for m == 3, their least-squares plane otherwise. A sample
 * outside [0, n), a degenerate or non-finite construction, or, with cos_limit > 0,
 * |normal . axis| < cos_limit make the hypothesis invalid: a row of zeros that counts 0.
 * A point is an inlier iff |((a x + b y) + c z) + d| < thresh, strictly.
 *   pts f64 [n,3]; samples i64 [H,m]; axis f64 [3] (unit) or NULL; planes f64 [H,4];
 *   counts i32 [H].
 * PYQSM_EINVAL, before any device is touched: m outside 3 ... 32, a threshold that is
 * not finite and > 0, a probability outside (0, 1], non-finite coordinates, H < 0,
 * P < 1, and n < m in the two segment calls. H == 0 is valid and finds nothing.
 */
int pyqsm_plane_models(const double* pts, int64_t n, const int64_t* samples, int64_t H, int32_t m,
                       const double* axis, double cos_limit, double* planes, int32_t device);
int pyqsm_plane_count(const double* pts, int64_t n, const double* planes, int64_t H, double thresh,
                      int32_t* counts, int32_t device);
/*
 * One plane. The rows are looked at in order; the first row with the largest count so far
 * wins (ties keep the lower row), and after every new winner with inlier fraction f the
 * rows beyond min(log(1 - probability) / log(1 - f^m), H) are not looked at (Open3D's
 * adaptive bound; none with probability == 1, or where f^m vanishes next to 1). *used = the
 * rows looked at, *best = the winning row (-1: no row has an inlier; then zeros and no inliers).
 *   plane_hyp: the winning hypothesis. plane_fit: the least-squares plane through its
 *   inliers from exact fixed-point moments, the same bits whatever the order of the
 *   points (plane_hyp with fewer than 3 inliers or a non-finite refit).
 *   inliers i64 [n] capacity, ascending; *n_inliers = their number.
 */
int pyqsm_segment_plane(const double* pts, int64_t n, const int64_t* samples, int64_t H, int32_t m,
                        double thresh, double probability, const double* axis, double cos_limit,
                        double plane_fit[4], double plane_hyp[4], int64_t* inliers, int64_t* n_inliers,
                        int64_t* best, int64_t* used, int32_t device);
/*
 * Up to P planes peeled off a cloud that stays on the device. Round r works on the points
 * not labelled yet, in ascending index order; sample j of hypothesis h is the alive point
 * number mulhi64(draws[r,h,j], n_alive) (the high 64 bits of the product), so the caller
 * need not know which points are left. A round is pyqsm_segment_plane on the alive points;
 * its inliers get label r. The call stops before a round with n_alive < m, at a round whose
 * winner has fewer than min_inliers inliers (it labels nothing), or after P rounds.
 *   draws u64 [P,H,m]; labels i32 [n] (-1: no plane); planes_fit / planes_hyp f64 [P,4],
 *   counts / best / used i64 [P] (zeros, 0, -1, 0 from row *n_planes on).
 */
int pyqsm_segment_planes(const double* pts, int64_t n, const uint64_t* draws, int64_t P, int64_t H,
                         int32_t m, double thresh, double probability, int64_t min_inliers,
                         const double* axis, double cos_limit, int32_t* labels, double* planes_fit,
                         double* planes_hyp, int64_t* counts, int64_t* best, int64_t* used,
                         int64_t* n_planes, int32_t device);

/* ---- Laplacian-contraction solve --------------------------------------- */
/*
 * One contraction solve of pyQSM/geometry/skeletonize.py:148-180
 * (least_squares_sparse): the reference stacks A = [L W_L ; W_H] (:164, the weights
 * scale the COLUMNS of L), so this minimises |L W_L x|^2 + |W_H (x - p)|^2 per
 * coordinate, i.e. (W_L L' L W_L + W_H^2) x = W_H^2 p, by a preconditioned conjugate
 * gradient over 3 right-hand sides that never forms L'L.
 *   L as CSR (indptr i32 [n+1], indices i32 [nnz], vals f64 [nnz]);
 *   wl, wh, f64 [n]; pts f64 [n,3] (also the start vector); out f64 [n,3]
 *   positive wl that is constant along every edge of L (uniform, as extract_skeleton
 *   produces it, or one value per connected block of a block-diagonal L): flexible
 *   CG preconditioned by B^-2, B = W_L L + W_H; stops when the preconditioned
 *   residual |B^-2 r| / |x|, an estimate of the relative error of x (B^-2 A has
 *   its spectrum in [1/2, 1] for uniform W_H), is <= rtol for every coordinate;
 *   any other wl: Jacobi-CG, stops when |r|/|b| <= rtol. Also stops after max_it sparse passes or when
 *   the estimate has stopped improving (attainable accuracy); in those two cases
 *   returns PYQSM_ENOCONV with the best iterate in `out`. `resid` always receives
 *   the true relative residuals |r|/|b| of the returned iterate.
 */
int pyqsm_lbc_solve(const int32_t* indptr, const int32_t* indices, const double* vals,
                    int64_t n, const double* wl, const double* wh, const double* pts,
                    double rtol, int32_t max_it, double* out, int32_t* iters,
                    double* resid, int32_t device);
/* y = L x for 3 columns at once (x, y f64 [n,3]); the SpMV the solve is built on. */
int pyqsm_spmv3(const int32_t* indptr, const int32_t* indices, const double* vals,
                int64_t n, const double* x, double* y, int32_t device);
/*
 * For tests: the multigrid hierarchy of B = diag(cw) L + diag(wh) that preconditions the B-solves
 * of pyqsm_lbc_solve, built by the function the solve calls (same environment switches), and one
 * cycle of it per right-hand side through both of its interfaces.
 *   L as CSR (symmetric, diagonal stored); cw, wh f64 [n]; rhs f64 [m, n, 3], m >= 0.
 *   meta i64 [108]: [0] levels, [1] coarsest solve (0 smoothing sweeps, 1 inverse made on the host,
 *   2 inverse made on the device), [2] rows of the inverse, [3] its leading dimension, [4..6] the
 *   elements the hierarchy takes in ibuf / dbuf / fbuf, [7] 1 when they were written; then four per
 *   level: rows, stored entries, aggregates (-1 on the last level), entries of A P (-1: no table).
 *   With fewer than two levels (no hierarchy the solve would use) only meta[0] is set.
 *   ibuf i32 [icap], level by level: indptr [n+1], indices [nnz]; with a coarser level agg [n],
 *   mptr [aggregates + 1], members [mptr's last]; with an A P table ap_ptr [n+1], ap_idx.
 *   dbuf f64 [dcap], level by level: vals [nnz], diag [n], dinv [n]; then the inverse as stored
 *   ([ld, ld]; the host-made one transposed). fbuf f32 [fcap]: ap_val of every level.
 *   A buffer that is too small: nothing is written or run, meta[4..6] say what to bring.
 *   x64 f64 [m, n, 3]: the cycle of the fp64 interface; x32 f32 [m, n, 3]: that of the fp32
 *   interface on the fp32 rounding of rhs; dots f64 [m, 2, 3]: rhs . x per column as the cycles'
 *   last kernel leaves it (fp64 interface, then fp32), partial slots folded as the solve folds them.
 */
int pyqsm_amg_probe(const int32_t* indptr, const int32_t* indices, const double* vals, int64_t n,
                    const double* cw, const double* wh, const double* rhs, int64_t m, int64_t* meta,
                    int32_t* ibuf, int64_t icap, double* dbuf, int64_t dcap, float* fbuf,
                    int64_t fcap, double* x64, float* x32, double* dots, int32_t device);
/* In-place clamp of every coordinate into [lo, hi] (skeletonize.py:291-296). */
int pyqsm_clamp(double* pts, int64_t n, const double lo[3], const double hi[3],
                int32_t device);

/* ---- fixed-radius queries -------------------------------------------------- */
/*
 * All points within `radius` of one centre (inclusive, d <= radius), ascending
 * indices: scipy KDTree(points).query_ball_point(center, r) as called at
 * pyQSM/utils/lib_integration.py:114-115 (find_neighbors_in_ball).
 *   out_idx i64 [n] capacity; *count = number written.
 */
int pyqsm_ball_query(const double* xyz, int64_t n, const double center[3], double radius,
                     int64_t* out_idx, int64_t* count, int32_t device);
/*
 * Union of the (at most k_cap nearest) neighbours within `radius` (strict,
 * d < radius) of every query point: the index set produced by
 * scipy KDTree(src).query(qry, k, distance_upper_bound=radius) at
 * pyQSM/geometry/reconstruction.py:238-244 and pyQSM/tree_isolation.py:126-131.
 *   mark u8 [n]: 1 for every source point some query selects;
 *   counts i32 [m]: neighbours each query selects (<= k_cap).
 */
int pyqsm_radius_mark(const double* src, int64_t n, const double* qry, int64_t m, double radius,
                      int32_t k_cap, uint8_t* mark, int32_t* counts, int32_t device);
/*
 * The padded tables themselves — what scipy KDTree(src).query(qry, k,
 * distance_upper_bound=radius) returns at pyQSM/geometry/reconstruction.py:238-240
 * and get_neighbors_kdtree(return_pcd=False) hands to pyQSM/canopy_metrics.py:238:
 * per query the (up to) k nearest source points with d < radius, ascending by
 * (distance, index); missing entries are padded with distance +inf and index n.
 *   idx i64 [m,k], dist f64 [m,k] (distances, not squared); 1 <= k <= 2048.
 */
int pyqsm_radius_knn(const double* src, int64_t n, const double* qry, int64_t m, double radius,
                     int32_t k, int64_t* idx, double* dist, int32_t device);
/*
 * pyqsm_radius_knn's neighbours reduced in the kernel: what pyQSM's expand_features_to_orig and
 * get_smoothed_features (canopy_metrics.py:236-252, 564-570) compute on the host from the padded
 * tables. The neighbours of query j are exactly the entries pyqsm_radius_knn(src, qry, radius, k)
 * returns for it: the same strict bound, d2 expression and (distance, index) order. values f64
 * [n, F] reduced over them into out f64 [m, F]: reducer 0 mean (sum from 0.0, one add at a time in
 * neighbour order, divided by the count: pyqsm_smooth_values' rule), 2 min, 3 max (NaN propagates
 * as in NumPy), 4 first (the nearest neighbour's row); anything else: PYQSM_EINVAL. A query with
 * no neighbour gets values[empty_row] (pyQSM falls back to row 0), or NaN when empty_row is -1.
 * counts i32 [m] (may be NULL): neighbours found, 0 to k. k in [1, 2048] and F in [1, 64]
 * (PYQSM_ERANGE); n up to 2^31 - 1; any m, served in chunks. No float atomics: every run gives
 * the same bits.
 */
int pyqsm_radius_reduce(const double* src, int64_t n, const double* qry, int64_t m, double radius, int32_t k,
                        const double* values, int32_t F, int32_t reducer, int64_t empty_row, double* out,
                        int32_t* counts, int32_t device);
/*
 * pyqsm_radius_mark with a label per query point: label[j] = the smallest label among
 * the query points that select source point j (-1: none). One call replaces one cycle
 * of the region growing of pyQSM/tree_isolation.py:207-256 (extend_seed_clusters), where
 * clusters are visited in index order and the first one to reach a free point keeps it.
 *   qry_label i32 [m] (>= 0); label i32 [n]; counts i32 [m] as in pyqsm_radius_mark.
 */
int pyqsm_radius_label(const double* src, int64_t n, const double* qry, int64_t m,
                       const int32_t* qry_label, double radius, int32_t k_cap, int32_t* label,
                       int32_t* counts, int32_t device);
/*
 * The whole region growing of pyQSM/tree_isolation.py:98-262 (extend_seed_clusters without
 * order_cutoff) in one call: the source, its grid, the ownership and the frontier stay on the device
 * for all cycles.
 *   src f64 [n,3]; owner_in i32 [n]: -1 free, else a cluster index < n_clusters;
 *   seed_xyz f64 [m,3] with seed_label i32 [m] in [0, n_clusters): the frontier of cycle 0 (the
 *   seed points need not be source points).
 * Cycle c: every frontier point of every cluster that is still growing selects its (at most k_cap
 * nearest) source points with d < radius: the rule of pyqsm_radius_mark to the bit (same grid, d2
 * expression, strict bound, k-th distance and tie rule). Owned points count towards the k nearest
 * but are not acquired. A free point selected in cycle c goes to the smallest cluster index among
 * the clusters that selected it in that cycle: owner_out = that index, cycle_out = c. What a
 * cluster acquired in a cycle is its next frontier. A cluster stops after a cycle in which it
 * acquired fewer than min_new points (it keeps them; pyQSM: 5), none included; a cluster without a
 * seed point never queries. The loop ends after `cycles` cycles, or when no cluster is growing.
 *   owner_out i32 [n], cycle_out i32 [n]: points never acquired keep owner_in and get cycle -1;
 *   finished i32 [n_clusters]: -1 if the cluster was still growing when the cycles ran out, else
 *     the number of cycles in which it queried (0 without a seed point);
 *   stats i64 [4] (may be NULL): cycles run, frontier queries served, points acquired, the most
 *     frontier queries served in one cycle.
 * n == 0, m == 0 or cycles == 0: answered on the host, no device is touched (an empty source
 * answers the seeds' first cycle with nothing: finished = 1). PYQSM_EINVAL: NULL pointers, a radius
 * that is not positive and finite, k_cap <= 0, min_new < 1, cycles < 0, an owner_in outside
 * [-1, n_clusters) or a seed_label outside [0, n_clusters); PYQSM_ERANGE: n or m of 2^31 or more.
 * Integer atomics only: every run gives the same bits, whatever the order of the seed points.
 */
int pyqsm_grow_clusters(const double* src, int64_t n, const int32_t* owner_in, const double* seed_xyz,
                        const int32_t* seed_label, int64_t m, int32_t n_clusters, double radius,
                        int32_t k_cap, int32_t cycles, int32_t min_new, int32_t* owner_out,
                        int32_t* cycle_out, int32_t* finished, int64_t* stats, int32_t device);

/* ---- cluster adjacency ------------------------------------------------------ */
/*
 * Which clusters of a labelled cloud touch which clusters of another, how closely and at how many
 * point pairs: the graph pyQSM/cluster_joining.py:126-164 (determine_adjacency) builds from one
 * cKDTree.sparse_distance_matrix(tree_j, threshold) per cluster pair, in one grid pass.
 *   src f64 [n,3] with src_label i32 [n] in [0, n_src_labels); tgt f64 [m,3] with tgt_label i32 [m]
 *   in [0, n_tgt_labels). A negative label means "ignore this point". A point pair counts when
 *   d2 = ((dx*dx) + dy*dy) + dz*dz <= threshold * threshold, both in fp64 (inclusive; zero counts).
 *   One row per cluster pair (a, b) with at least one such point pair, ascending by (a, b):
 *   a, b i32; min_d2 f64 (the minimum SQUARED distance; sqrt of it is cKDTree's value); pairs i64
 *   (point pairs within the threshold). Each array holds `capacity` rows: at most that many are
 *   written, *count is the number found, and a caller who gets count > capacity calls again.
 * flags: PYQSM_ADJ_SAME_CLOUD  source and target are one cloud (tgt, tgt_label, m, n_tgt_labels are
 *          ignored): only rows with a < b, every unordered point pair counted once, pairs of equal
 *          label skipped;
 *        PYQSM_ADJ_WITNESS     also src_idx, tgt_idx i64 [capacity]: the closest point pair, on ties
 *          the smallest source index, then the smallest target index (both NULL otherwise);
 *        PYQSM_ADJ_NO_CACHE    every point pair goes to the table with atomics of its own (same
 *          result; for measuring what the per-lane accumulation saves).
 * stats i64 [2] or NULL: distance tests evaluated, pairs of table atomics issued.
 * Nothing labelled on either side: *count = 0 and no device is touched. Non-finite coordinates,
 * threshold <= 0 or not finite, a label >= its bound: PYQSM_EINVAL. n_src_labels * n_tgt_labels
 * above 2^26: PYQSM_ERANGE (split the sources by label range; rows stay sorted).
 */
#define PYQSM_ADJ_SAME_CLOUD 1
#define PYQSM_ADJ_WITNESS 2
#define PYQSM_ADJ_NO_CACHE 4
int pyqsm_cluster_adjacency(const double* src, const int32_t* src_label, int64_t n, int32_t n_src_labels,
                            const double* tgt, const int32_t* tgt_label, int64_t m, int32_t n_tgt_labels,
                            double threshold, int32_t flags, int64_t capacity, int32_t* a, int32_t* b,
                            double* min_d2, int64_t* pairs, int64_t* src_idx, int64_t* tgt_idx, int64_t* count,
                            int64_t* stats, int32_t device);

/* ---- radius graph: exact degrees and pair list ------------------------------------ */
/*
 * The graph whose vertices are the points of a cloud and whose edges join two points within a radius
 * r of each other: what pyQSM builds with KDTree.query_pairs(r) and a Python loop over the pairs
 * (pyQSM/utils/lib_integration.py:48-71 get_pairs), thresholds at a percentile of the degree
 * (scripts/graph_based_leaf_id.py:28-38).
 * One rule for both calls, cKDTree's at p = 2 and pyqsm_cluster_adjacency's: {i, j}, i != j, is
 * an edge when d2 = ((dx*dx) + dy*dy) + dz*dz <= r*r, everything in fp64 without contraction; the
 * bound is inclusive and coincident points are joined.
 *   xyz f64 [n,3].
 * pyqsm_radius_degrees: radii f64 [R], 1 <= R <= 8, in any order, repeats allowed; degree i32 [R, n]:
 *   degree[k * n + i] = the number of edges at point i for radii[k] (the point itself is not counted);
 *   n_pairs i64 [R] = half the sum of row k, the length of query_pairs(radii[k]). O(n) memory: no pair is
 *   stored. ONE grid is built, at the largest radius, and every d2 is computed once and compared with
 *   all R bounds: a radius far below the largest pays for the largest one's candidates (27 cells of
 *   the largest radius per point); call it on its own when that matters.
 *   stats i64 [2] or NULL: distance tests evaluated, candidates staged through LDS.
 * pyqsm_radius_pairs: pairs i32 [capacity, 2]: every edge once as (i, j), i < j in the caller's
 *   indices, the list ascending by (i, j), the same bits on every run. At most `capacity` rows are
 *   written (the first of the sorted list), *count is the number found, and a caller who gets
 *   count > capacity calls again with room (capacity = 0 only counts). More than 2^31 - 256 pairs
 *   with capacity > 0: PYQSM_ERANGE.
 * Both: n == 0 is answered on the host, no device is touched (n_pairs = 0, *count = 0). PYQSM_EINVAL: NULL pointers, non-finite coordinates, a radius that is not
 * positive and finite; PYQSM_ERANGE: R outside [1, 8], n of 2^31 - 256 or more.
 * Integer atomics only (per-block sums of degrees): every run gives the same bits.
 * pyqsm_radius_components: the connected components of the graph at every radius of radii f64 [R], 1 <= R <= 8,
 *   any order, repeats allowed, ranked by (size descending, smallest member ascending): what pyQSM takes
 *   from sorted(rustworkx.connected_components(g), key=len, reverse=True) over the pair list
 *   (scripts/graph_based_leaf_id.py:80-97, qsm_generation.py:526-556). Row k of every output is for radii[k]:
 *   component i32 [R, n] the rank of point i's component; sizes i32 [R, n], the first n_components[k]
 *   entries of row k valid (the others are left as they were): sizes[k * n + s] = the points of rank s;
 *   members i32 [R, n] or NULL: the point indices ascending by (component, index), so the points of rank s
 *   are the slice between the prefix sums of sizes; n_components i64 [R]. No pair is stored: O(n) memory.
 *   One grid at the largest radius, one union pass and one ranking per radius. The same bits on every run:
 *   a set's label is its smallest member whatever order the unions arrive in, the sizes are integer sums.
 *   They are also pyqsm_dbscan's clusters at eps = r, min_pts = 1, numbered differently.
 *   n == 0: n_components = 0, no device touched; errors as pyqsm_radius_degrees'.
 */
int pyqsm_radius_degrees(const double* xyz, int64_t n, const double* radii, int32_t R, int32_t* degree,
                         int64_t* n_pairs, int64_t* stats, int32_t device);
int pyqsm_radius_pairs(const double* xyz, int64_t n, double radius, int64_t capacity, int32_t* pairs,
                       int64_t* count, int32_t device);
int pyqsm_radius_components(const double* xyz, int64_t n, const double* radii, int32_t R, int32_t* component,
                            int32_t* sizes, int32_t* members, int64_t* n_components, int32_t device);

/* ---- projected area: the exact 2-D alpha shape of lattice points --------------- */
/*
 * For every segment (an independent cloud) of integer lattice points the total area of the cells of
 * its Delaunay subdivision whose circumradius^2 <= a2 (cocircular points form one cell, so the
 * subdivision is unique): what delaunay_2d(alpha).area approximates in pyQSM's
 * viz/ray_casting.py project_pcd, computed with integer predicates only.
 *   ij i32 [n,2] lattice coordinates; seg_start i64 [n_seg + 1], ascending from 0 to n: points of
 *   different segments never meet. a2: alpha^2 in lattice units^2, inclusive bound. Coincident
 *   points of a segment are merged: the lowest index takes part.
 *   twice_area i64 [n_seg]: twice the area in lattice units^2; n_live i64 [n_seg]: points after
 *   merging; n_boundary i64 [n_seg]: directed boundary edges (kept cell on the left, none on the right).
 * flags: PYQSM_ALPHA_BOUNDARY  *edges receives the boundary edges of all segments, i64 [sum of
 *          n_boundary, 2] pairs of indices into ij, grouped by segment in segment order, ascending by
 *          (a, b) inside one; allocated by the library, released with pyqsm_free; NULL when there is
 *          none (edges itself may be NULL without the flag).
 * max_tests: the call is refused with PYQSM_ERANGE, before the edge pass, when the estimated number
 *   of point-against-edge tests, the sum over the points of (points in the 3 x 3 cell stencil)^2,
 *   exceeds it; <= 0: PYQSM_ALPHA_DEFAULT_MAX_TESTS, ten seconds at the 4.0e11 tests per second measured on
 *   one MI355X; the executed tests never exceed the estimate.
 * stats i64 [5] or NULL: estimated tests, executed tests, comparisons decided by the 128-bit
 *   fallback, directed edges within reach, merged duplicates.
 * A segment with fewer than three distinct points, or with all points on one line, has area 0 and
 * no boundary; when every segment is like that no device is touched. The extent of a segment above
 * 2^20 lattice units on an axis, a2 above 2^40, a seg_start that does not run from 0 to n: PYQSM_EINVAL.
 */
#define PYQSM_ALPHA_BOUNDARY 1
#define PYQSM_ALPHA_DEFAULT_MAX_TESTS 4000000000000LL
int pyqsm_alpha_area(const int32_t* ij, int64_t n, const int64_t* seg_start, int64_t n_seg, uint64_t a2,
                     int64_t max_tests, int32_t flags, int64_t* twice_area, int64_t* n_live, int64_t* n_boundary,
                     int64_t** edges, int64_t* stats, int32_t device);

/* ---- mesh checks: edge table, clusters, manifoldness, self-intersection -------- */
/*
 * What pyQSM's geometry/mesh_processing.py asks of Open3D before a mesh is cast at, by a contract
 * of integer decisions and a fixed output order. Everything is decided by
 * vertex INDEX, as Open3D does: nothing is welded.
 *
 * pyqsm_mesh_topology
 *   tris i32 [n_tris,3]; verts f64 [n_verts,3] or NULL (then no areas: *cluster_area stays NULL).
 *   Allocated by the library, released with pyqsm_free (NULL when n_tris == 0):
 *     *edges i32 [E,2]       the undirected edges (a < b), ascending by (a, b)
 *     *edge_count i32 [E]    triangles at each edge
 *     *edge_flags u8 [E]     1 boundary (one triangle); 2 more than two triangles; 4 exactly two
 *                            triangles that traverse the edge in the SAME direction (a winding
 *                            conflict as the mesh is given)
 *     *cluster_n i64 [C], *cluster_area f64 [C]
 *   tri_cluster i32 [n_tris]: triangles that share an edge are connected; the clusters are numbered
 *     by ascending smallest member triangle. The area of a triangle is
 *     0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v1 - v0) x (v2 - v0), every component a*b - c*d
 *     without fused multiply-adds; a cluster's areas are added in a fixed order without
 *     floating-point atomics (the same bits on every run), |sum - exact| <= (n_c + 4) 2^-52 exact.
 *   vertex_flags u8 [n_verts]: 1 where the triangles at the vertex are not ONE set under "share an
 *     edge that contains this vertex" (Open3D's fan test); a vertex without triangles is manifold.
 *   summary i64 [8]: E, boundary edges, edges with more than two triangles, same-direction edges,
 *     non-manifold vertices, clusters, orientable (0 / 1), vertices without a triangle.
 *     Orientable: some choice of flips makes every two triangles at a shared edge traverse it in
 *     opposite directions; an edge with more than two triangles rules that out.
 *   An index outside [0, n_verts) or a triangle that repeats an index: PYQSM_EINVAL;
 *   n_tris >= 2^29: PYQSM_ERANGE; both before any launch. n_tris == 0 launches nothing.
 *
 * pyqsm_mesh_self_intersections
 *   ijk i32 [n_verts,3] lattice coordinates, at most 2^20 units of extent per axis (PYQSM_EINVAL
 *   beyond: every orient3d determinant then fits int64). A pair i < j of triangles is reported iff
 *   they share no vertex index, neither is degenerate (its three lattice vertices collinear or
 *   coincident) and the two closed triangles have a common point: piercing, touching at a vertex,
 *   an edge or a face, coplanar overlap. Integer predicates only.
 *   *n_pairs: the number of such pairs; tri_hit u8 [n_tris]: 1 for a triangle of some pair.
 *   flags: PYQSM_MESH_PAIRS  *pairs receives i32 [*n_pairs,2], ascending by (i, j), never truncated;
 *            allocated by the library, released with pyqsm_free; NULL when there is none (pairs
 *            itself may be NULL without the flag).
 *   max_tests: n_tris (n_tris - 1) / 2 above it is refused with PYQSM_ERANGE before any launch;
 *     <= 0: PYQSM_MESH_DEFAULT_MAX_TESTS = 1.6e13, ten seconds at 1.6e12 box tests per second: one
 *     MI355X sweeps the 1.25e11 pairs of 500 000 triangles at 1.66e12 pairs per second on an unwelded
 *     canopy soup and at 2.17e12 on a welded closed surface (tools/mesh_perf.py,
 *     profiles/mesh_perf.jsonl); the lower rate, rounded down. A value of 0
 *     would mean "no default": max_tests <= 0 is then refused with PYQSM_EINVAL.
 *   stats i64 [6] or NULL: pairs considered, pairs whose boxes overlap, of those skipped for a
 *     shared index, degenerate triangles, exact tests run, pairs reported.
 *   The sweep works on tiles of PYQSM_MESH_TILE_ROWS triangles. More than 2^26 triangles: PYQSM_ERANGE.
 */
#define PYQSM_MESH_PAIRS 1
#define PYQSM_MESH_TILE_ROWS 256
#define PYQSM_MESH_DEFAULT_MAX_TESTS 16000000000000LL
int pyqsm_mesh_topology(const int32_t* tris, int64_t n_tris, int64_t n_verts, const double* verts, int32_t** edges,
                        int32_t** edge_count, uint8_t** edge_flags, int32_t* tri_cluster, int64_t** cluster_n,
                        double** cluster_area, uint8_t* vertex_flags, int64_t* summary, int32_t device);
int pyqsm_mesh_self_intersections(const int32_t* ijk, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                                  int32_t flags, int64_t max_tests, int64_t* n_pairs, int32_t** pairs,
                                  uint8_t* tri_hit, int64_t* stats, int32_t device);

/* ---- mesh hole filling: boundary loops, minimum-area patches ------------------- */
/*
 * What pyQSM's geometry/surf_recon.py meshfix asks of pymeshfix's fill_small_boundaries, by a contract of
 * its own with a fixed output order; not MeshFix's triangulation. Everything is by
 * vertex INDEX, nothing is welded, no vertex is added. tris, n_tris, n_verts and their refusals as in
 * pyqsm_mesh_topology; n_tris == 0 launches nothing; a mesh without a boundary has no loops.
 *
 * Half-edge h = 3 t + k runs from corner k of triangle t to corner (k + 1) % 3; it is a boundary half-edge
 * when its undirected edge has exactly one triangle. succ(h), h = (a -> b): g = next(h) in h's triangle;
 * while g is not a boundary half-edge, g = next(twin(g)), which leaves b again; the first boundary g. The
 * walk stops where g's edge has more than two triangles or two that run the same way (no twin): h then
 * lies on an OPEN CHAIN, as does every half-edge that leads to it or is led to by nothing. The walk is
 * capped at the number of triangle corners at b. The cycles of succ are the LOOPS.
 *
 * A loop of length L is listed v_0 .. v_{L-1} in the fill direction: (v_{m+1} -> v_m) is a boundary
 * half-edge of the mesh, so a new triangle traverses each boundary edge against the triangle that is
 * there. v_0 is the loop's smallest vertex index; where it occurs more than once, the occurrence whose
 * half-edge leaving it has the smaller h. Loops are numbered ascending by (v_0, that h).
 *   *loop_ptr i32 [n_loops + 1], *loop_verts i32 [loop_ptr[n_loops]]
 *   *loop_flags u8 [n_loops]: 1 some vertex occurs more than once; 2 L > max_edges; 0: the loop is filled.
 *     max_edges <= 0: PYQSM_FILL_MAX_LOOP; above it: PYQSM_EINVAL.
 *
 * The patch of a filled loop, p_m = verts[v_m] in fp64: W(i, i+1) = 0; for d = 2 .. L-1, i = 0 .. L-1-d,
 * k = i + d, j ascending in (i, k): w = (W(i,j) + W(j,k)) + A(i,j,k); a later j replaces an earlier one
 * only when strictly smaller. A = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (p_j - p_i) x (p_k - p_i),
 * every component a*b - c*d without fused multiply-adds: the area of pyqsm_mesh_topology. Rows in
 * pre-order of the split tree: emit(i,k) writes (v_i, v_j, v_k), j = split(i,k), then emit(i,j), then
 * emit(j,k). L - 2 rows per filled loop, the loops ascending.
 *   *loop_area f64 [n_loops]: W(0, L-1); 0 where not filled
 *   *new_tris i32 [*n_new,3], *new_loop i32 [*n_new]: the rows and the loop each belongs to
 * Loops of at most PYQSM_FILL_WAVE_MAX edges are patched by one wave each, longer ones by one block each;
 * the result does not depend on the class.
 *
 * stats i64 [8]: boundary half-edges, loops, loops filled, loops with a repeated vertex, loops too long,
 *   half-edges on open chains, new rows of area exactly 0.0, diagonals of the patches that are already
 *   an edge of the mesh. Neither of the last two changes the result: the caller re-runs the checks.
 *   pyqsm_mesh_boundary_loops fills the first two and the sixth.
 * Buffers are allocated by the library, released with pyqsm_free and NULL when empty. The same bytes on
 * every run.
 */
#define PYQSM_FILL_MAX_LOOP 128
#define PYQSM_FILL_WAVE_MAX 32
int pyqsm_mesh_boundary_loops(const int32_t* tris, int64_t n_tris, int64_t n_verts, int64_t* n_loops,
                              int32_t** loop_ptr, int32_t** loop_verts, int64_t* stats, int32_t device);
int pyqsm_mesh_fill_holes(const int32_t* tris, int64_t n_tris, int64_t n_verts, const double* verts, int32_t max_edges,
                          int64_t* n_loops, int32_t** loop_ptr, int32_t** loop_verts, uint8_t** loop_flags,
                          double** loop_area, int64_t* n_new, int32_t** new_tris, int32_t** new_loop, int64_t* stats,
                          int32_t device);

/* ---- surface reconstruction: exact ball pivoting of lattice points ------------- */
/*
 * The triangles a ball of radius rho can rest on from the normals' side (the alpha-exposed facets of
 * the alpha shape, alpha = rho): an order-free, exact stand-in for Open3D's
 * create_from_point_cloud_ball_pivoting, whose front depends on its traversal.
 *   ijk i32 [n,3] lattice coordinates (at most 2^31 - 1 units of extent per axis); normals i16 [n,3],
 *   rint(n * 2^14). rho2 u64 [n_levels]: rho^2 in lattice units^2, ascending, each in
 *   [1, PYQSM_RECON_MAX_RHO2] (PYQSM_EINVAL beyond, with the factor by which the quantum must grow).
 * An oriented triple (a, b, c), n = (b - a) x (c - a), is emitted at a level iff the three vertex
 * normals have a strictly positive dot product with n, the ball of radius rho through a, b, c with
 * its centre on the +n side exists (circumradius <= rho) and holds no other point strictly inside.
 * Points exactly on the ball: if all of them lie in the triangle's plane the triple is kept iff its
 * smallest index is the smallest among them too and none lies strictly beyond the edge opposite that
 * vertex (the fan from the smallest index); otherwise it is kept and counted in stats[4].
 * Levels after the first accept a triple only if none of its vertices is inner (has triangles, and
 * every incident half-edge has its reverse) and none of its directed half-edges exists already.
 *   *tris receives i32 [*n_tris,4] rows (a, b, c, level), a the smallest index, ascending by
 *   (a, b, c); allocated by the library, released with pyqsm_free; NULL when there is none. The same
 *   bytes on every run. More than 8 n + 1024 triangles, or more than 2^26 points: PYQSM_ERANGE.
 * max_tests: the call is refused with PYQSM_ERANGE when the estimated pair tests of a level, the sum over
 *   the points of (points in the 27-cell stencil)^2, exceed it; <= 0: PYQSM_RECON_DEFAULT_MAX_TESTS = 1e12,
 *   ten seconds at the 1.1e11 estimated pair tests per second of the triangle pass measured on one MI355X
 *   (profiles/recon_perf.jsonl), rounded down. The estimate needs the level's grid:
 *   the binning kernels of the levels up to the refused one have run by then, but no triangle pass of ANY
 *   level has (with several radii every level is binned and estimated first).
 * stats i64 [8] or NULL: estimated pair tests (all levels so far), ball tests run (candidates x stencil),
 *   of those classified by the wide integers, candidate triples, triangles kept with a tie point off
 *   their plane, the largest stencil, the most points in one cell, blocks launched. All but one are the
 *   same on every run; the count of wide-integer classifications is not: a lane stops at the first point
 *   inside its ball, and the order of the points within a grid cell, which decides what it meets before
 *   that, is the binning's arrival order. No triangle depends on it.
 * Fewer than three points: no triangle, no device work.
 */
#define PYQSM_RECON_MAX_RHO2 4194304ULL /* 2^22: rho <= 2^11 lattice units */
#define PYQSM_RECON_CHUNK 1024
#define PYQSM_RECON_SLICE 16
#define PYQSM_RECON_DEFAULT_MAX_TESTS 1000000000000LL
int pyqsm_ball_pivot(const int32_t* ijk, const int16_t* normals, int64_t n, const uint64_t* rho2, int32_t n_levels,
                     int64_t max_tests, int64_t* n_tris, int32_t** tris, int64_t* stats, int32_t device);

/* ---- 3-D alpha shape: exact boundary triangles and volume of lattice points ------ */
/*
 * What Open3D's create_from_point_cloud_alpha_shape extracts from the Delaunay tetrahedra of circumradius
 * below alpha, by a contract of its own that needs no tetrahedra and no normals.
 *   ijk i32 [n,3] lattice coordinates (at most 2^31 - 1 units of extent per axis, at most 2^26 points).
 *   seg_start i64 [n_seg + 1], from 0 to n, ascending, or NULL (one segment, n_seg is ignored): a triple
 *   and the points that block it belong to one segment; the result equals running every segment alone.
 *   rho2 = alpha^2 in lattice units^2, in [1, PYQSM_RECON_MAX_RHO2] (PYQSM_EINVAL beyond, with the factor by
 *   which the quantum must grow).
 * A triple {a, b, c} of one segment with n = (b - a) x (c - a) != 0 and circumradius <= alpha has two balls
 * of radius alpha through it, B+ on the +n side and B-. A ball is empty when no other point of the segment
 * is strictly inside. kind 1 (regular): exactly one ball is empty and they are two (H > 0); the row is
 * oriented so that n points to the empty ball, out of the solid. kind 2 (singular): both are empty and
 * H > 0; written only with faces == PYQSM_ALPHA3_ALL, with b < c, and no part of the volume.
 * Ties are ball pivoting's: a point on a ball does not block; a point on both balls in the triangle's plane
 * drops the triple when its index is below a's or it lies strictly beyond the edge opposite a; a triple
 * kept with a point off its plane exactly on an empty ball is counted in stats[4], and the surface may then
 * fail to close: vol6 means a volume only when that counter is 0. Coincident points are not merged.
 *   *rows receives i32 [*n_rows,4] rows (a, b, c, kind), a the smallest index, ascending by (a, b, c), hence
 *   grouped by segment; allocated by the library, released with pyqsm_free; NULL when there is none. More than
 *   16 n + 1024 rows: PYQSM_ERANGE.
 *   vol6 u64 [n_seg,2] (low, high half): the sum of det(a - o, b - o, c - o) over the regular rows of the
 *   segment, o its first point, as a 128-bit two's complement: six times the enclosed volume in lattice
 *   units^3, from integer sums only. The same bytes on every run, rows and vol6 alike.
 * max_tests: as pyqsm_ball_pivot's: PYQSM_ERANGE before the triangle pass when the estimate, the sum over
 *   the points of (points in the 27-cell stencil)^2, exceeds it; <= 0: PYQSM_ALPHA3_DEFAULT_MAX_TESTS = 4e12,
 *   ten seconds at the 4.1e11 estimated pair tests per second of the triangle pass measured on one MI355X
 *   (forest cloud, alpha = 2 mean spacings; 4.6e11 at 4 spacings; profiles/alpha3_perf.jsonl, DESIGN.md section
 *   27), rounded down. The pass lists no stencil^2 pairs, so it serves the same estimate four times as fast as
 *   pyqsm_ball_pivot's.
 * stats i64 [8] or NULL: estimated pair tests, ball tests run (candidates x neighbours within 2 alpha), of
 *   those classified by the wide integers, candidate triples, rows kept with an off-plane tie, the largest
 *   stencil, the most points in one cell, work items. Only the count of wide-integer classifications may
 *   differ between runs (a lane stops asking about a ball at the first point inside it).
 * Fewer than three points: no row, no device work.
 */
#define PYQSM_ALPHA3_REGULAR 0
#define PYQSM_ALPHA3_ALL 1
#define PYQSM_ALPHA3_CHUNK 1024
#define PYQSM_ALPHA3_SLICE 16
#define PYQSM_ALPHA3_DEFAULT_MAX_TESTS 4000000000000LL
int pyqsm_alpha_shape3(const int32_t* ijk, int64_t n, const int64_t* seg_start, int64_t n_seg, uint64_t rho2,
                       int32_t faces, int64_t max_tests, int64_t* n_rows, int32_t** rows, uint64_t* vol6,
                       int64_t* stats, int32_t device);

/* ---- farthest-point down-sampling ---------------------------------------- */
/*
 * Stands in for open3d PointCloud.farthest_point_down_sample(num_samples) as
 * called by extract_topology at pyQSM/geometry/skeletonize.py:127-132.
 *   out_idx i32 [num_samples]: indices in selection order, the first being
 *   start_index (Open3D starts at 0); each next one is the point farthest from
 *   everything selected so far (squared distance in fp64, lowest index on ties).
 */
int pyqsm_fps(const double* xyz, int64_t n, int64_t num_samples, int64_t start_index,
              int32_t* out_idx, int32_t device);

/* ---- point-cloud Laplacian ---------------------------------------------- */
/*
 * Stands in for robust_laplacian.point_cloud_laplacian(pts, mollify_factor,
 * n_neighbors) at pyQSM/geometry/skeletonize.py:253-255,341-343: kNN -> PCA
 * normal -> tangent-plane projection -> local Delaunay fan per point -> union
 * of fan triangles -> mollified cotangent Laplacian and lumped mass, both / 3.
 *   On success the indptr / indices / vals out-parameters hold a CSR matrix
 *   (symmetric, zero row sums) owned by the library: release each with
 *   pyqsm_free. mass f64 [n].
 */
int pyqsm_pc_laplacian(const double* xyz, int64_t n, int32_t k, double moll,
                       int64_t* nnz, int32_t** indptr, int32_t** indices, double** vals,
                       double* mass, int32_t device);
/*
 * The same for several clouds stacked into one array (the per-cluster calls of
 * pyQSM/qsm_generation.py:182-316 batched into one build): points [seg_start[s],
 * seg_start[s+1]) are cloud s, n_seg clouds, seg_start i64 [n_seg + 1] from 0 to n.
 * The mollification length (max(0, largest triangle slack + moll x mean edge length))
 * is taken per cloud, as n_seg separate calls would. The clouds must lie apart (further
 * than any k-neighbourhood reaches) for the result to be block diagonal; the caller
 * arranges that (extract_skeleton_batch moves every cloud to its own lattice cell).
 */
int pyqsm_pc_laplacian_seg(const double* xyz, int64_t n, const int64_t* seg_start, int64_t n_seg,
                           int32_t k, double moll, int64_t* nnz, int32_t** indptr,
                           int32_t** indices, double** vals, double* mass, int32_t device);

/* ---- the whole contraction loop, resident in HBM ------------------------------ */
/*
 * extract_skeleton of pyQSM/geometry/skeletonize.py:240-373 as ONE call: Laplacian ->
 * contraction solve -> clamp (:291-296) -> weights (:329-335) -> next Laplacian, up to
 * max_iter times, with the points, the matrix and the weights staying on the device
 * (the Python loop moves ~200 MB over PCIe per step at one million points). The loop's
 * bookkeeping is the reference's (W_H updated with the mass of the Laplacian just used,
 * volume ratio lagging one step, stop when a solve changes nothing or returns only NaN).
 *   xyz f64 [n,3]; seg_start i64 [n_seg+1] (NULL with n_seg = 1): several clouds stacked
 *   into one array are contracted together — one build and one block-diagonal solve per
 *   step — while weights, clamp box, volume ratio and termination stay per cloud;
 *   lo, hi f64 [n_seg,3]: the clamp box of every cloud (the reference takes the min / max
 *   bound of the oriented bounding box, :240-241); rtol, solver_max_it as pyqsm_lbc_solve.
 *   out_pts, total_shift f64 [n,3]; steps f64 [max(max_iter,1), n, 3] or NULL: the shift of
 *   every step (zero for clouds that had stopped); n_steps i32 [n_seg]: steps each cloud
 *   took; solve_iters i32 / solve_resid f64 / solve_ok u8 [max(max_iter,1)] (each may be
 *   NULL): per solve, as pyqsm_lbc_solve reports them; *n_solves: solves run.
 */
int pyqsm_extract_skeleton(const double* xyz, int64_t n, const int64_t* seg_start, int64_t n_seg,
                           int32_t k, double moll, int32_t max_iter, double termination_ratio,
                           double contraction_factor, double attraction_factor,
                           double max_contraction, double max_attraction, const double* lo,
                           const double* hi, double rtol, int32_t solver_max_it, double* out_pts,
                           double* total_shift, double* steps, int32_t* n_steps,
                           int32_t* solve_iters, double* solve_resid, uint8_t* solve_ok,
                           int32_t* n_solves, int32_t device);

/* ---- filters in front of the oriented bounding box's convex hull ----------------- */
/*
 * pyQSM/geometry/skeletonize.py:240-241 clamps the contracted points into
 * pcd.get_oriented_bounding_box().get_min_bound() / get_max_bound(); Open3D builds that box from
 * a PCA of the convex hull's vertices. Qhull over every point of a scan is 0.3 s per million
 * points; these two calls cut its input down to ~1 % without changing the hull:
 *   pyqsm_extreme_points: idx i64 [n_dirs] = the point with the largest x . dirs[d] (dirs f64
 *   [n_dirs,3]; lowest index on ties);
 *   pyqsm_outside_halfspaces: eq f64 [n_planes,4] = (a, o) of half-spaces a . x + o <= 0 (the
 *   facets of a small polytope whose corners are points of the cloud, scipy.spatial.ConvexHull
 *   .equations); idx i64 [capacity n] receives, ascending, every i with a . x_i + o >= -margin for
 *   some plane — the points that are not strictly inside — and *count their number. A point
 *   strictly inside such a polytope is strictly inside the cloud's hull, so the hull of the
 *   listed points has the same vertices. At most 256 planes.
 */
int pyqsm_extreme_points(const double* xyz, int64_t n, const double* dirs, int32_t n_dirs,
                         int64_t* idx, int32_t device);
int pyqsm_outside_halfspaces(const double* xyz, int64_t n, const double* eq, int32_t n_planes,
                             double margin, int64_t* idx, int64_t* count, int32_t device);

/*
 * Host-side helper of that loop, exported so that it can be checked without a GPU: the mean of
 * v[0..n) with NumPy's summation order (pairwise in blocks of 128 with eight accumulators, one
 * 8192-element buffer after the other, as np.add.reduce runs over a contiguous array with the
 * default buffer size), i.e. bit for bit what np.mean(M.diagonal())
 * of pyQSM/geometry/skeletonize.py:265,349 returns. The initial Laplacian weight is
 * 10^3 c sqrt(mean M): one ulp of difference there is amplified by the loop to millimetres
 * after twenty steps, so the native loop takes the mean the way the Python loop gets it.
 * n <= 0: *out = NaN.
 */
int pyqsm_mean_f64(const double* v, int64_t n, double* out);

/* ---- cloud cleaning: voxel down-sampling and statistical outlier removal ---------- */
/*
 * Open3D's PointCloud.voxel_down_sample and remove_statistical_outlier as clean_cloud at
 * pyQSM/geometry/point_cloud_processing.py:97-127 applies them (also qsm_generation.py:99-101,447,
 * canopy_metrics.py:187,275,380). Open3D's source is not at hand: the semantics below are
 * recollected from Open3D, parity unpinned; tests/clean_restatement.py defines them.
 *
 * pyqsm_voxel_down_sample: xyz f64 [n,3], colors f64 [n,3] or NULL, voxel_size > 0 and finite.
 *   vmin = min_bound - voxel_size / 2; key = floor((p - vmin) / voxel_size) per axis (IEEE fp64
 *   division); PYQSM_ERANGE when the three index ranges span more than 2^62 cells. One output
 *   row per occupied voxel, ordered by the smallest input index it holds (Open3D's order is an
 *   unordered_map's); its value is the sum of the members in ascending index order, from 0.0,
 *   one add at a time, divided by their count (colours alike). *m = rows; *out_xyz (and
 *   *out_colors when colors is given) are library buffers of m rows, released with pyqsm_free.
 *   Optional trace: inverse i64 [n] = output row of every point; offsets i64 [capacity n+1] and
 *   members i64 [n] = the members of row r, ascending, at members[offsets[r] .. offsets[r+1]).
 */
int pyqsm_voxel_down_sample(const double* xyz, int64_t n, const double* colors, double voxel_size,
                            int64_t* m, double** out_xyz, double** out_colors, int64_t* inverse,
                            int64_t* offsets, int64_t* members, int32_t device);
/*
 * pyqsm_stat_outlier: k = min(nb_neighbors, n) <= 192 nearest points of every point, the point
 * itself included (d2 = ((dx*dx) + dy*dy) + dz*dz); avg[i] = (sum of sqrt(d2), ascending, one add
 * at a time from 0.0) / k; mean = (sum of the positive avg) / n, std = sqrt(sum over positive avg
 * of (avg - mean)^2 / (n - 1)), thr = mean + std_ratio * std (both sums fixed-order device
 * reductions: the same bits on every run). Keeps i iff 0 < avg[i] < thr.
 *   keep i64 [capacity n]: kept indices ascending, *n_keep of them; avg f64 [n] or NULL;
 *   stats f64 [3] = (mean, std, thr) or NULL. nb_neighbors >= 1 and std_ratio > 0.
 */
int pyqsm_stat_outlier(const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio,
                       int64_t* keep, int64_t* n_keep, double* avg, double* stats, int32_t device);
/*
 * pyqsm_clean_cloud: the loop of clean_cloud with the cloud resident in HBM: the voxel step
 * when voxel_size > 0 (0: off), then `iters` rounds of statistical outlier removal with
 * int(neighbors) neighbours, after each round neighbors *= 2 and ratio /= 1.5; the kept points
 * are gathered into a fresh array between rounds. iters = 0 returns the voxel step alone (the
 * Python clean_cloud returns its input instead when the statistical step is off, as pyQSM does).
 *   *m = points left; *out_xyz = library buffer of m rows, released with pyqsm_free.
 */
int pyqsm_clean_cloud(const double* xyz, int64_t n, double voxel_size, double neighbors, double ratio,
                      int32_t iters, int64_t* m, double** out_xyz, int32_t device);

/* ---- normals: estimation, consistent orientation, the stem stage ----------------------- */
/*
 * Open3D's PointCloud.estimate_normals and orient_normals_consistent_tangent_plane as get_stem_pcd
 * applies them (pyQSM/qsm_generation.py:71-120; also fit.py:93, surf_recon.py:107,158,
 * mesh_processing.py:201). Recollected from Open3D, parity unpinned; tests/normals_restatement.py
 * defines the contract.
 *
 * pyqsm_estimate_normals: xyz f64 [n,3]. Neighbourhood of i: with radius > 0 and finite (hybrid),
 *   the up to max_nn nearest points with d2 < radius^2, max_nn in [1, 256]; otherwise (KNN) the
 *   min(max_nn, n) nearest, max_nn in [1, 192] (PYQSM_ERANGE outside). The point itself counts;
 *   d2 = ((dx*dx) + dy*dy) + dz*dz in fp64; ties go to the lower index, so the neighbours are
 *   ascending by (d2, index). Covariance on offsets o = p_j - p_i: m = (sum o) / N,
 *   C = (sum (o - m)(o - m)^T) / N, each sum from 0.0 one add at a time in neighbour order. The
 *   normal is the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi, pca.hpp). Fewer
 *   than 3 neighbours or C == 0: prev_normals[i] when given, else (0, 0, 1). Sign: flipped when
 *   dot(n, prev_normals[i]) < 0, or without prev_normals (NULL) when n_z < 0.
 *   normals f64 [n,3] out.
 */
int pyqsm_estimate_normals(const double* xyz, int64_t n, double radius, int32_t max_nn,
                           const double* prev_normals, double* normals, int32_t device);
/*
 * pyqsm_orient_normals_tangent_plane: the min(k, n) nearest of every point (the point itself
 *   counted, its self edge dropped), k in [1, 192], as undirected edges of weight
 *   w = 1 - |(nx*mx + ny*my) + nz*mz| ordered by (w, min(i,j), max(i,j)): the unique minimum
 *   spanning forest. A point's sign relative to its tree's root is the XOR along the tree path of
 *   (dot(n_i, n_j) < 0) on the input normals. Each component is rooted at its highest point
 *   (largest z, lowest index), whose normal is flipped when n_z < 0. No EMST edges: components of
 *   the kNN graph are oriented independently. oriented f64 [n,3] out; *rounds (may be NULL) =
 *   Boruvka rounds that merged components.
 */
int pyqsm_orient_normals_tangent_plane(const double* xyz, int64_t n, const double* normals, int32_t k,
                                       double* oriented, int32_t* rounds, int32_t device);
/*
 * pyqsm_stem_cloud: get_stem_pcd's device part, one upload and one download: crop (keep
 *   z > min z + crop_offset; no crop when that bound is exactly 0, as pyQSM's crop), normals
 *   (radius, max_nn, prev_normals of all n points or NULL), orientation (orient_k), then
 *   filter_by_norm's test -angle_cutoff < degrees(atan(nz / sqrt(nx^2 + ny^2))) < angle_cutoff
 *   (angle 0 when nx = ny = 0). keep i64 [capacity n]: input indices of the kept points,
 *   ascending; normals f64 [capacity n,3]: their oriented normals; *m = how many.
 */
int pyqsm_stem_cloud(const double* xyz, int64_t n, const double* prev_normals, double crop_offset,
                     double radius, int32_t max_nn, int32_t orient_k, double angle_cutoff,
                     int64_t* keep, double* normals, int64_t* m, int32_t device);

/* ---- branch tracing: k-means, silhouette, the ball step with exclusion ------------------- */
/*
 * pyQSM's sphere_step (qsm_generation.py:182-316) and the kmeans it reaches through
 * choose_and_cluster (math_utils/fit.py:58-85, 168-214). tests/sphere_restatement.py states the
 * contract; DESIGN.md section 10.
 *
 * Chunk sum (the reduction of the centroid sums and of the mean silhouette): 256 consecutive values
 * per chunk (zeros past the end), each group of four summed ((v0 + v1) + v2) + v3, the 64 group sums
 * added pairwise (neighbours first, six levels); the chunk totals added one at a time from 0.0.
 *
 * pyqsm_kmeans: scipy.cluster.vq.kmeans2(xy, init, iters, minit='matrix') on the x, y of the m
 *   points xyz f64 [m,3], k in [1, PYQSM_KMEANS_MAX_K]. vq: label = argmin over c of
 *   (dx*dx) + dy*dy with d = p - centroid, ties to the lowest c. Update: the chunk sums of each
 *   centroid's members' x and y over their count; a centroid without members keeps its position.
 *   init f64 [k,2]; centroids f64 [k,2] after the last update; labels i32 [m] of the last
 *   assignment (which precedes the last update), as kmeans2 returns them.
 */
#define PYQSM_KMEANS_MAX_K 8
#define PYQSM_KMEANS_MAX_Q 4
#define PYQSM_SILHOUETTE_MAX_K 65536
int pyqsm_kmeans(const double* xyz, int64_t m, int32_t k, int32_t iters, const double* init,
                 double* centroids, int32_t* labels, int32_t device);
/*
 * pyqsm_silhouette: sklearn.metrics.silhouette_score of xyz f64 [m,3] under labels i32 [m] in
 *   [0, k), k <= PYQSM_SILHOUETTE_MAX_K. d(i,j) = sqrt(((dx*dx) + dy*dy) + dz*dz), dx = x_i - x_j,
 *   correctly rounded. For every point and every label c the sum of d(i,j) over the members j of c,
 *   one add at a time from 0.0 in ascending j. a = own sum / (n_own - 1); b = the smallest
 *   sum / n_c over the other labels with members; s_i = (b - a) / max(a, b), 0 for a singleton and
 *   for 0/0. *score = chunk sum of s over m. *n_present = labels with members; the labelling is
 *   valid iff 2 <= *n_present <= m - 1 (sklearn raises otherwise; here every s_i and *score are
 *   0). samples f64 [m] (may be NULL) = s_i.
 */
int pyqsm_silhouette(const double* xyz, int64_t m, const int32_t* labels, int32_t k, double* score,
                     int32_t* n_present, double* samples, int32_t device);
/*
 * pyqsm_kmeans_select: the candidates of pyQSM's kmeans in one pass: for q < nk, k = k0 + q
 *   (1 <= k0, k0 + nk - 1 <= PYQSM_KMEANS_MAX_K, nk <= PYQSM_KMEANS_MAX_Q) pyqsm_kmeans with
 *   `iters` iterations from init (f64, the nk initial centroid sets packed: [k0 + (k0+1) + ...][2]),
 *   then pyqsm_silhouette of the 3-D points under its labels. labels i32 [nk,m], scores f64 [nk],
 *   present i32 [nk] come back in one copy. The _dev form takes device-resident xyz.
 */
int pyqsm_kmeans_select(const double* xyz, int64_t m, int32_t k0, int32_t nk, int32_t iters,
                        const double* init, int32_t* labels, double* scores, int32_t* present,
                        int32_t device);
int pyqsm_kmeans_select_dev(const double* xyz_dev, int64_t m, int32_t k0, int32_t nk, int32_t iters,
                            const double* init, int32_t* labels, double* scores, int32_t* present,
                            int32_t device);
/*
 * pyqsm_ball_excl_dev: the points i of the device cloud xyz_dev f64 [n,3] with
 *   ((dx*dx) + dy*dy) + dz*dz <= radius^2 (pyqsm_ball_query's inclusive bound) and found_dev[i] == 0
 *   (u8 [n]), compacted by scan: idx_dev i64 [capacity n] ascending, out_xyz_dev f64 [capacity n,3]
 *   their coordinates (contiguous: the input of pyqsm_dbscan_dev_ex and pyqsm_kmeans_select_dev).
 *   *count (host) = how many; reading it synchronises.
 * pyqsm_mark_found_dev: found_dev[idx[j]] = 1 for the cnt host indices idx (those outside [0, n)
 *   are skipped). Synchronises.
 */
int pyqsm_ball_excl_dev(const double* xyz_dev, int64_t n, const uint8_t* found_dev, const double center[3],
                        double radius, int64_t* idx_dev, double* out_xyz_dev, int64_t* count,
                        int32_t device);
int pyqsm_mark_found_dev(uint8_t* found_dev, int64_t n, const int64_t* idx, int64_t cnt, int32_t device);

/* ---- geometric features and neighbour smoothing ------------------------------------------ */
/*
 * jakteristics' compute_features and pyQSM's smooth_feature (pyQSM/exploration.py:62-90,
 * utils/algo.py:8-22). Recollected from jakteristics (Hackel et al. 2016), parity unpinned;
 * tests/features_restatement.py defines the contract; DESIGN.md section 11.
 *
 * pyqsm_geometric_features: xyz f64 [n,3]. Neighbourhood of i: every j (i included) with
 *   ((dx*dx) + dy*dy) + dz*dz <= radius^2 in fp64 (metric 2), or (|dx| + |dy|) + |dz| <= radius
 *   (metric 1); when more than max_k qualify, the max_k first by (distance, index). Covariance on
 *   the offsets o = p_j - p_i: C = (sum o o^T - (sum o)(sum o)^T / N) / (N - 1), the sums exact in
 *   128-bit fixed point (every term rounded to 2^-61 of the largest possible offset), so the
 *   result is reproducible bit for bit and independent of the input order. lambda1 >= lambda2 >=
 *   lambda3 (clamped to >= 0), e3 the unit eigenvector of lambda3 with e3_z >= 0. feature_ids
 *   [n_features] (1 to 32 columns) in jakteristics' FEATURE_NAMES numbering: 0 eigenvalue_sum,
 *   1 omnivariance, 2 eigenentropy, 3 anisotropy, 4 planarity, 5 linearity, 6 PCA1, 7 PCA2,
 *   8 surface_variation, 9 sphericity, 10 verticality, 11 nx, 12 ny, 13 nz. N < 3 or
 *   lambda1 == 0: NaN. out f64 [n, n_features]; counts i32 [n] (may be NULL): N before the cap.
 *   radius <= 0 or not finite, a bad metric or feature id: PYQSM_EINVAL; max_k < 1 or
 *   n_features outside [1, 32]: PYQSM_ERANGE.
 */
int pyqsm_geometric_features(const double* xyz, int64_t n, double radius, int32_t max_k, int32_t metric,
                             const int32_t* feature_ids, int32_t n_features, double* out, int32_t* counts,
                             int32_t device);
/*
 * pyqsm_smooth_values: the k nearest of each query among the n points xyz f64 [n,3], ascending by
 *   (d2, index) with d2 = ((dx*dx) + dy*dy) + dz*dz; qry f64 [m,3], or NULL for the points
 *   themselves (m == n; each point then counts itself). k in [1, 192] (PYQSM_ERANGE), k > n:
 *   PYQSM_EINVAL. values f64 [n, F] reduced over each query's neighbours into out f64 [m, F]:
 *   reducer 0 mean (fp64 sum in neighbour order, divided by k), 1 median (np.median: the mean of
 *   the two middle values for even k), 2 min, 3 max; NaN propagates as in NumPy. reducer -1: no
 *   reduction (values and out may be NULL). idx i32 [m, k] (may be NULL unless reducer is -1):
 *   the neighbour table.
 */
int pyqsm_smooth_values(const double* xyz, int64_t n, const double* qry, int64_t m, const double* values,
                        int32_t F, int32_t k, int32_t reducer, double* out, int32_t* idx, int32_t device);

/* ---- tree-ensemble inference -------------------------------------------------------------- */
/*
 * Inference of a fitted scikit-learn tree ensemble (pyQSM/exploration.py:460-538: the
 * RandomForestClassifier that labels points wood / leaf / epiphyte). Training stays on the host.
 * The contract is scikit-learn's own arithmetic (tree/_tree.pyx _apply_dense,
 * ForestClassifier.predict_proba with n_jobs=1) and is matched bit for bit;
 * tests/forest_restatement.py restates it in NumPy; DESIGN.md section 12.
 *
 *   row x (float32 [F]; NaN allowed, +-inf is the caller's to reject), per tree from the root: at
 *   an internal node (feature f, threshold t f64, missing_go_to_left): x[f] NaN goes left when
 *   the flag is set, else right; otherwise left iff (double)x[f] <= t. A leaf has left == -1.
 *   leaves[i, k] = the leaf's node number within tree k. acc = 0 (f64 [C]); for k = 0 .. T-1 in
 *   that order acc += value[leaf_k, :]; proba = acc / T (one division per entry); label = the
 *   first maximum of proba. No floating-point atomics, no re-associated partial sums: every run
 *   gives the same bits.
 *
 * Limits of the device layout (an 8-byte node record: float32 threshold; missing flag, 8-bit
 * feature and 22-bit child slot packed; one f64 accumulator per class and lane; a block's rows in
 * LDS). The float32 threshold is the largest float32 not above t, which decides every float32 x
 * exactly as (double)x <= t does.
 */
#define PYQSM_FOREST_MAX_FEATURES 64
#define PYQSM_FOREST_MAX_CLASSES 32
#define PYQSM_FOREST_MAX_TREE_NODES 4194304u /* per tree; 2^31 - 1 in the whole forest */
/*
 * pyqsm_forest_create: the T trees' nodes concatenated, tree k in [tree_offsets[k],
 *   tree_offsets[k+1]) (tree_offsets i64 [T+1], [0] == 0), children as node numbers within their
 *   tree (left == right == -1: leaf), value f64 [nodes, C]. The topology is validated on the host
 *   before anything is uploaded: children in range and reached once (so every path ends in a
 *   leaf), 0 <= feature < F, thresholds not NaN, leaf values finite: PYQSM_EINVAL otherwise;
 *   beyond the limits above: PYQSM_ERANGE. Nodes no path reaches are ignored. The forest is
 *   re-laid out, uploaded once to `device` and stays there until pyqsm_forest_free (NULL: no-op).
 * pyqsm_forest_info: info[0..7] = T, C, F, node records on the device, leaves, depth of the
 *   deepest leaf (root = 0), device bytes, nodes of each tree staged in LDS.
 * pyqsm_forest_stage: how many of each tree's first (breadth-first) nodes the kernel reads from
 *   LDS: 0, 512, 1024 or 2048 (default: 1024 up to 16 features and 8 classes, where a lane walks
 *   two rows at a time, else 512). Changes speed only, never a result.
 * pyqsm_forest_predict: X f32 [n, F] on the host; proba f64 [n, C], label i32 [n] (class index)
 *   and leaves i32 [n, T] on the host, each may be NULL. Rows go through the device in chunks that
 *   fit the arena; offsets are 64-bit (n * T may exceed 2^31).
 */
int pyqsm_forest_create(const int64_t* tree_offsets, const int32_t* left, const int32_t* right,
                        const int32_t* feature, const double* threshold, const uint8_t* missing_left,
                        const double* value, int32_t T, int32_t C, int32_t F, int32_t device, void** forest);
int pyqsm_forest_free(void* forest);
int pyqsm_forest_info(const void* forest, int64_t info[8]);
int pyqsm_forest_stage(void* forest, int32_t staged_nodes);
int pyqsm_forest_predict(const void* forest, const float* X, int64_t n, double* proba, int32_t* label,
                         int32_t* leaves);

/* ---- voxel-grid occupancy ------------------------------------------------------------------ */
/*
 * Open3D's VoxelGrid.create_from_point_cloud + check_if_included, the step with which pyQSM asks
 * which points of a full-resolution tile belong to a voxelised tree (pyQSM/geometry/
 * reconstruction.py:266-355, tree_isolation.py:465-516, canopy_metrics.py:635-639). Recollected
 * from Open3D (VoxelGrid::CreateFromPointCloud / GetVoxel / CheckIfIncluded), parity unpinned;
 * tests/voxelgrid_restatement.py defines the contract; DESIGN.md section 14.
 *
 * pyqsm_voxel_grid_create: origin[a] = min_bound[a] - voxel_size * 0.5; a point's voxel index is
 *   floor((p[a] - origin[a]) / voxel_size) with a true IEEE fp64 division: the arithmetic of
 *   pyqsm_voxel_down_sample, so a cloud's grid and its down-sampling have the same voxels in the
 *   same row order. One voxel per occupied index, rows ordered by the smallest input index they
 *   hold (Open3D's order is an unordered_map's). With colors f64 [n,3] the voxel colour is the mean
 *   of its members in ascending index order, one add at a time from 0.0, divided by the count.
 *   dims[a] = the largest index + 1. voxel_size not positive and finite, or a non-finite
 *   coordinate: PYQSM_EINVAL; a dimension above 2^31 - 1 or more than 2^62 cells: PYQSM_ERANGE;
 *   all of these before any device is touched. n == 0: a grid without voxels, origin
 *   -voxel_size / 2, dims 0, in which nothing is included. The grid stays on `device` until
 *   pyqsm_voxel_grid_free (NULL: no-op); any number of grids may be alive.
 * pyqsm_voxel_grid_info: every out-parameter may be NULL.
 * pyqsm_voxel_grid_voxels: grid_index i32 [M,3] and colors f64 [M,3] in row order (each may be
 *   NULL; colors of a grid created without: PYQSM_EINVAL).
 * pyqsm_voxel_grid_query: per query f[a] = floor((q[a] - origin[a]) / voxel_size); included iff
 *   0 <= f[a] < dims[a] on every axis and that voxel exists. A NaN or infinite coordinate is never
 *   included. (Open3D casts f to int, which wraps far outside the box: out of contract here.)
 *   included u8 [m]; row i32 [m]: the voxel's row, -1 if none; idx i64 [capacity m]: the ascending
 *   query indices that are included, or with PYQSM_VOX_INVERT those that are not; *count: their
 *   number. Every output may be NULL. The host form streams qry through the device in chunks
 *   (any m, 64-bit offsets; PYQSM_VOX_CHUNK in the environment lowers the chunk's size); the _dev
 *   form takes device arrays and writes device arrays (*count stays a host value).
 */
#define PYQSM_VOX_INVERT 1
int pyqsm_voxel_grid_create(const double* xyz, int64_t n, const double* colors, double voxel_size,
                            int32_t device, void** grid);
int pyqsm_voxel_grid_free(void* grid);
int pyqsm_voxel_grid_info(const void* grid, double origin[3], double* voxel_size, int64_t dims[3],
                          int64_t* n_voxels, int64_t* device_bytes);
int pyqsm_voxel_grid_voxels(const void* grid, int32_t* grid_index, double* colors);
int pyqsm_voxel_grid_query(const void* grid, const double* qry, int64_t m, int32_t flags,
                           uint8_t* included, int32_t* row, int64_t* idx, int64_t* count);
int pyqsm_voxel_grid_query_dev(const void* grid, const double* qry_dev, int64_t m, int32_t flags,
                               uint8_t* included_dev, int32_t* row_dev, int64_t* idx_dev, int64_t* count);

/* ---- skeleton graph and cylinder table ----------------------------------------------------- */
/*
 * What follows the contraction and the farthest-point sampling (pyQSM/geometry/skeletonize.py:36-146,
 * :375-441): the spanning forest of the kNN graph, the collapse of its degree-2 chains, one radius
 * per chain and the sampled cylinder surfaces. tests/topology_restatement.py states the contract;
 * DESIGN.md section 15.
 *
 * pyqsm_skeletal_forest: minimum spanning forest of the undirected kNN graph of xyz f64 [m,3]:
 *   {i,j} is an edge when j is among the k nearest of i (itself excluded) or i among those of j,
 *   weighted with the d2 of pyqsm_knn (the smaller of the two directions' values, should they
 *   differ). Padded entries are no edges. A pair at distance exactly 0 unites the components of its
 *   ends but is never listed, as in SciPy's minimum_spanning_tree on explicit zeros (its Kruskal pass
 *   joins across them, its result drops them); so exact duplicates never get an edge between them
 *   and the listed edges alone may leave them apart. Edges are ordered by
 *   (d2, packed (min, max)), a strict total order that refines the order by sqrt(d2): the forest is
 *   unique, and a minimum spanning forest of the square-root weights as well. k in [1, 192]
 *   (PYQSM_ERANGE, before any device is touched). edges i32 [capacity m - 1, 2] with a < b in
 *   every row, rows ascending by (a, b); d2 f64 [capacity m - 1]; *n_edges; *rounds (may be
 *   NULL): Boruvka rounds that hooked a component. The listed forest has m - *n_edges components. The
 *   same bits on every run. m < 2: no edge, nothing launched. The _dev form takes and fills device
 *   arrays; the counts stay host values.
 * pyqsm_collapse_chains: edges i32 [e,2] over nodes 0 .. m-1 MUST form a forest (an end outside
 *   [0, m) or a self-loop: PYQSM_EINVAL; a walk that meets no end within m steps, as on a ring
 *   through a kept node, too - a ring of degree-2 nodes alone is not noticed and not reported).
 *   kept i32 [capacity m]: the nodes of degree != 2, ascending. Every maximal run of degree-2 nodes
 *   between kept nodes a < b is a chain: chain_ends i32 [capacity e, 2] rows (a, b) ascending,
 *   chain_ptr i64 [capacity e + 1], members i32 [capacity m] in walking order from a to b; an edge
 *   between two kept nodes is a chain without members. counts[3]: kept nodes, chains, members.
 * pyqsm_chain_radii: radius[c] = mean over the members s of chain c of |shift[s]|, or of
 *   |shift[index_map[s]]| when index_map i32 [n_map] is not NULL; shift f64 [n,3]; the norm is
 *   sqrt((x x + y y) + z z); the terms are added in the order of NumPy's pairwise summation (eight
 *   running sums up to 128 terms, halves above), the contract being the rounding bound of a sum of
 *   positive terms, |r - mean| <= (len + 4) 2^-52 mean. A chain without members gets
 *   0. An index out of range: PYQSM_EINVAL.
 * pyqsm_cylinder_surfaces: params f64 [q,14] = centre, unit axis, u, v (3 each), radius, height;
 *   cos_sin f64 [40] = the 20 cosines, then the 20 sines. Per cylinder the 100 x 20 points
 *   (centre + radius (cos u + sin v)) + along axis, along = np.linspace(-height / 2, height / 2, 100),
 *   rounded to millimetres (rint(x 1000) / 1000.0), distinct rows in lexicographic order, of equal
 *   rows the first in (level, angle) order. surface_ptr i64 [q + 1]; *points_out f64 [*total_out, 3]
 *   is allocated by the library (release with pyqsm_free; NULL when q == 0). A cylinder more than
 *   2^21 mm across: PYQSM_ERANGE; a coordinate that is not finite: PYQSM_EINVAL.
 */
int pyqsm_skeletal_forest(const double* xyz, int64_t m, int32_t k, int32_t* edges, double* d2, int64_t* n_edges,
                          int32_t* rounds, int32_t device);
int pyqsm_skeletal_forest_dev(const double* xyz_dev, int64_t m, int32_t k, int32_t* edges_dev, double* d2_dev,
                              int64_t* n_edges, int32_t* rounds, int32_t device);
int pyqsm_collapse_chains(const int32_t* edges, int64_t e, int64_t m, int32_t* kept, int32_t* chain_ends,
                          int64_t* chain_ptr, int32_t* members, int64_t* counts, int32_t device);
int pyqsm_collapse_chains_dev(const int32_t* edges_dev, int64_t e, int64_t m, int32_t* kept_dev,
                              int32_t* chain_ends_dev, int64_t* chain_ptr_dev, int32_t* members_dev, int64_t* counts,
                              int32_t device);
int pyqsm_chain_radii(const double* shift, int64_t n, const int64_t* chain_ptr, int64_t n_chains,
                      const int32_t* members, const int32_t* index_map, int64_t n_map, double* radius,
                      int32_t device);
int pyqsm_cylinder_surfaces(const double* params, int64_t q, const double* cos_sin, int64_t* surface_ptr,
                            double** points_out, int64_t* total_out, int32_t device);

/* ---- stem width: order statistics of the pairwise distances ------------------- */
/*
 * For every segment (an independent cloud) the elements of given ranks of its sorted pairwise
 * distances, scipy.spatial.distance.pdist bit for bit, without the distances ever being stored: what
 * pyQSM's canopy_metrics.width_at_height reads off np.percentile(pdist(slab[:, :2]), q)
 * (DESIGN.md section 21).
 *   pts f64 [n, dim], dim 2 or 3 (anything else: PYQSM_EINVAL), finite and of magnitude below 1e150
 *   (a precondition, not checked); seg_start i64 [n_seg + 1], ascending from 0 to n (PYQSM_EINVAL
 *   otherwise). Segment s with n_s points has M_s = n_s (n_s - 1) / 2 pairs i < j, written to n_pairs
 *   i64 [n_seg]. The key of a pair is d2 = (dx*dx) + (dy*dy), for dim 3 with + (dz*dz) added last, in
 *   fp64 without contraction; keys are ordered by their bit pattern.
 *   ranks i64 [n_seg, n_ranks], 0-based; values f64 [n_seg, n_ranks]: values[s, r] = sqrt of the key
 *   of rank ranks[s, r] among segment s's keys in ascending order. A rank < 0 marks an unused slot,
 *   which receives 0.0; a rank >= M_s: PYQSM_EINVAL (so a segment with M_s = 0 takes unused slots
 *   only). Equal ranks in one segment are fine. n_ranks from 0 to PYQSM_PDIST_MAX_RANKS, above it
 *   PYQSM_EINVAL.
 *   max_pair i64 [n_seg, 2] or NULL: the pair (i, j), i < j, of indices local to the segment with the
 *   largest key, of equal keys the smallest (i, j) in lexicographic order; (-1, -1) when M_s = 0.
 * max_pairs: the call is refused with PYQSM_ERANGE, before any launch, when the sum of M_s exceeds
 *   it; <= 0: PYQSM_PDIST_DEFAULT_MAX_PAIRS, ten seconds of the eight passes at the 9.3e11 pair
 *   evaluations per second measured on one MI355X (profiles/width_perf.jsonl, case "single", n = 100000).
 * stats i64 [3] or NULL: the sum of M_s, the pair evaluations executed (every pass evaluates every pair
 *   once), the passes run.
 * Memory is O(n + n_seg * n_ranks * 256); nothing is read back between the passes; all counters are
 * integers summed by integer atomics, so every run gives the same bits. When every M_s is 0 no device
 * is touched.
 */
#define PYQSM_PDIST_MAX_RANKS 32
#define PYQSM_PDIST_DEFAULT_MAX_PAIRS 1200000000000LL
int pyqsm_pdist_select(const double* pts, int64_t n, int32_t dim, const int64_t* seg_start, int64_t n_seg,
                       const int64_t* ranks, int32_t n_ranks, int64_t max_pairs, double* values, int64_t* n_pairs,
                       int64_t* max_pair, int64_t* stats, int32_t device);

/* ---- epiphyte split: percentile cuts of a per-row key, k-means++ clumps ------------------- */
/*
 * The two stages of pyQSM's canopy_metrics.identify_epiphytes between the contraction's first shift
 * and the batched alpha-shape area (tests/epiphyte_restatement.py states the
 * contract in NumPy).
 *
 * pyqsm_select_values: the elements of given ranks of the sorted keys of n rows.
 *   v f64 [n, width], width 1 or 3. key: a component 0 <= key < width, or PYQSM_KEY_NORM (width 3):
 *   sqrt(((x*x) + (y*y)) + (z*z)), correctly rounded, no contraction. Keys order as the doubles do,
 *   negative ones included; -0.0 is keyed as +0.0 (and comes back as +0.0). A NaN anywhere in v:
 *   PYQSM_EINVAL. ranks i64 [n_ranks], 0-based, n_ranks from 0 to PYQSM_PDIST_MAX_RANKS; values f64
 *   [n_ranks]: values[r] = the key of rank ranks[r] in ascending order. A rank < 0 marks an unused
 *   slot, which receives 0.0; a rank >= n: PYQSM_EINVAL. n == 0 is answered on the host.
 *   A radix selection as pyqsm_pdist_select's: keys recomputed from the rows in each of eight 8-bit
 *   passes, integer histograms, nothing read back between the passes, memory O(n + n_ranks * 256).
 *   The _dev form takes device rows.
 * pyqsm_split_above_dev: the rows i with cmp(key(row i), threshold), cmp 0 >, 1 >=, 2 <, 3 <=, of the
 *   device rows v_dev, selected by scan: idx_dev i64 [capacity n] (may be NULL) their indices,
 *   ascending; out_rows_dev f64 [capacity n, 3] row i of rows_dev f64 [n, 3] for each of them (both
 *   may be NULL). *count (host) = how many; reading it synchronises. A NaN threshold: PYQSM_EINVAL.
 * pyqsm_shift_components: the three-way split of identify_epiphytes in one call. shift f64 [n, 3].
 *   thresholds[0] = P(q_mag) of the row norms; the rows with norm > thresholds[0] are "high";
 *   thresholds[1] = P(q_z) of the high rows' z (NaN when there is none). labels u8 [n]: 0 norm not
 *   above thresholds[0]; 1 high and z > thresholds[1] (leaf); 2 the other high rows (epiphyte).
 *   counts i64 [3] = rows per label. P(q) is NumPy's default percentile of m values: with
 *   v = (m - 1) * (q / 100), lo = floor(v), t = v - lo, a and b the order statistics of ranks lo and
 *   min(lo + 1, m - 1): a + (b - a) * t, b - (b - a) * (1 - t) where t >= 0.5, a where t == 0; taken
 *   once, on the host, from two selected values. q outside [0, 100] or a NaN in shift: PYQSM_EINVAL.
 *   n == 0: NaN thresholds, zero counts, no device work. The _dev form takes device shift and labels.
 */
#define PYQSM_KEY_NORM (-1)
int pyqsm_select_values(const double* v, int64_t n, int32_t width, int32_t key, const int64_t* ranks, int32_t n_ranks,
                        double* values, int32_t device);
int pyqsm_select_values_dev(const double* v_dev, int64_t n, int32_t width, int32_t key, const int64_t* ranks,
                            int32_t n_ranks, double* values, int32_t device);
int pyqsm_split_above_dev(const double* v_dev, int64_t n, int32_t width, int32_t key, int32_t cmp, double threshold,
                          const double* rows_dev, int64_t* idx_dev, double* out_rows_dev, int64_t* count,
                          int32_t device);
int pyqsm_shift_components(const double* shift, int64_t n, double q_mag, double q_z, uint8_t* labels,
                           double* thresholds, int64_t* counts, int32_t device);
int pyqsm_shift_components_dev(const double* shift_dev, int64_t n, double q_mag, double q_z, uint8_t* labels_dev,
                               double* thresholds, int64_t* counts, int32_t device);
/*
 * pyqsm_kmeans_pp: k-means of n points x f64 [n, d], d 1, 2 or 3, into 1 <= k <= PYQSM_KMEANSPP_MAX_K
 *   centres, n >= k (anything else: PYQSM_EINVAL), modelled on scikit-learn 1.7's
 *   KMeans(init="k-means++", n_init=1, algorithm="lloyd"). "Chunk sum" is the reduction stated above
 *   pyqsm_kmeans. The coordinates are finite (a precondition, not checked).
 *   Centring: mu_j = chunk sum of column j / n; all work is on x - mu;
 *     tol_abs = tol * ((s_0 + s_1 + s_2) / d), s_j = chunk sum of (x_j - mu_j)^2 / n, added in this
 *     order; mu is added back to the centres at the end.
 *   Distances: ((dx*dx) + dy*dy) + dz*dz in fp64, d = point - centre, always direct; the nearest
 *     centre is the argmin, ties to the lowest centre.
 *   Seeding: greedy k-means++ with T = 2 + int(ln k) trials per step. The caller draws the random
 *     numbers: `first`, the first centre's point, and u f64 [(k - 1) * T] uniforms in [0, 1), n_u of
 *     them (PYQSM_EINVAL otherwise). closest_i = the squared distance to the nearest chosen centre;
 *     a chunk total is the chunk sum of 256 consecutive closest; pot = the chunk totals added one at a
 *     time from 0.0. Step c = 1 .. k - 1, trial t: r = u[(c - 1) T + t] * pot. The chunk is the first
 *     whose cumulative total (the totals added in order from 0.0) is >= r, the last chunk if none is;
 *     inside it closest is added one value at a time to the cumulative total before the chunk, and the
 *     candidate is the first point at which the sum is >= r, the chunk's last point if none is. A
 *     trial's potential is the chunk totals of min(closest, squared distance to the candidate) added
 *     in order; the smallest wins, ties to the earlier trial. pot == 0 thus selects point 0.
 *   Lloyd: assign; per centre the masked chunk sums of each coordinate (a non-member counts 0.0), the
 *     chunk totals added in chunk order, over the member count give the new centre; a centre without
 *     members keeps its place (scikit-learn relocates it). After every update, in this order: labels
 *     equal to the previous iteration's: stop (strict convergence); the sum over the centres, in order
 *     from 0.0, of ((ex*ex) + ey*ey) + ez*ez, e = new - old centre, <= tol_abs: stop; max_iter
 *     iterations done: stop. Unless the stop was strict, the points are assigned once more to the final
 *     centres. (scikit-learn squares the rounded norm of e and sums pairwise: the same up to rounding.)
 *   labels i32 [n]; centres f64 [k, d]; *inertia = chunk sum of the squared distances to the labelled
 *   centres; *n_iter; *n_empty = centres without a member in labels; seeds i64 [k] the seeding's points.
 *   Iterations are queued in bursts (4, 4, 8, 16, then 32) behind a device-side "done" word, so the
 *   later ones of a burst are no-ops, and one small record is read per burst. No float atomics: every run gives the same bits. The _dev form takes device points.
 */
#define PYQSM_KMEANSPP_MAX_K 64
int pyqsm_kmeans_pp(const double* x, int64_t n, int32_t d, int32_t k, int64_t first, const double* u, int64_t n_u,
                    int32_t max_iter, double tol, int32_t* labels, double* centres, double* inertia, int32_t* n_iter,
                    int32_t* n_empty, int64_t* seeds, int32_t device);
int pyqsm_kmeans_pp_dev(const double* x_dev, int64_t n, int32_t d, int32_t k, int64_t first, const double* u,
                        int64_t n_u, int32_t max_iter, double tol, int32_t* labels, double* centres, double* inertia,
                        int32_t* n_iter, int32_t* n_empty, int64_t* seeds, int32_t device);

/* ---- convex hull: exact facets of lattice points, batched ---------------------- */
/*
 * The convex hull of every segment (an independent cloud) of integer lattice points, decided by int64
 * predicates only (csrc/hull_exact.hpp): what scipy.spatial.ConvexHull(points).simplices
 * and the hull behind pcd.get_oriented_bounding_box() are in pyQSM, with a fixed answer on degenerate input.
 *   ijk i32 [n,3] lattice coordinates; seg_start i64 [n_seg + 1], ascending from 0 to n. A segment may
 *   span at most 2^20 units on every axis (PYQSM_EINVAL beyond, before any launch): every orient3d
 *   determinant of differences is then below 6 * 2^60 < 2^63.
 * Which triangles: coincident points of a segment are merged, the lowest index takes part. A plane through
 *   three non-collinear points of the segment with no point strictly outside it is a facet plane; the points
 *   on it span a convex polygon whose extreme points are its vertices (points inside the polygon or inside
 *   one of its edges are not). With v0 the vertex of lowest index the facet gives one triangle (v0, x, y)
 *   for every directed polygon edge x -> y, counter-clockwise seen from outside, that does not contain v0.
 *   In general position every facet is one triangle and the rows are Qhull's simplices as a set.
 * Output, allocated by the library and released with pyqsm_free, NULL after an error:
 *   *tris i32 [T,3]: indices into ijk; in every row (a, b, c) a is the smallest and (b - a) x (c - a)
 *     points out of the hull; rows ascend by (a, b, c) inside a segment, segments in segment order.
 *   *tri_ptr i64 [n_seg + 1]: the rows of segment s are tri_ptr[s] .. tri_ptr[s + 1].
 *   dim i32 [n_seg] (the caller's): the affine dimension of the segment's distinct points, -1 for an empty
 *     segment. A segment with dim < 3 has no rows; when every segment is like that no device is touched
 *     (*tris stays NULL, *tri_ptr is all zero).
 *   The same bytes on every run.
 * How: in front, the extreme points of a segment along 26 fixed directions and four affinely independent
 *   points are wrapped into a small polytope, and every point strictly inside it is dropped; the survivors
 *   are wrapped in rounds of open directed edges, each facet handled as a unit.
 * max_tests: the running count of orient tests (one per point and pass of an open edge) is checked after every
 *   round; above max_tests the call ends with PYQSM_ERANGE. <= 0: PYQSM_HULL_DEFAULT_MAX_TESTS, ten seconds at
 *   the 2.0e11 tests per second measured on one MI355X (profiles/hull_perf.jsonl, the 100 000-point shell), rounded down. The plane tests of
 *   the prefilter (at most 56 per point) are not counted. The rounds are bounded by the facet count (every
 *   round with an open edge closes one); beyond 2 C + 8 rounds for C candidates the call returns PYQSM_EHIP.
 *   A facet polygon with more than PYQSM_HULL_MAX_FACET_VERTS vertices: PYQSM_ERANGE.
 * stats i64 [PYQSM_HULL_N_STATS] or NULL: candidates left after the prefilter, rounds of the main wrap, orient
 *   tests run (both wraps), facets with more than three points on their plane, merged duplicates among the
 *   candidates, rounds of the prefilter's wrap. All of them are the same on every run.
 */
#define PYQSM_HULL_N_STATS 6
#define PYQSM_HULL_MAX_FACET_VERTS 1024
#define PYQSM_HULL_DEFAULT_MAX_TESTS 2000000000000LL
int pyqsm_convex_hull(const int32_t* ijk, int64_t n, const int64_t* seg_start, int64_t n_seg, int64_t max_tests,
                      int32_t** tris, int64_t** tri_ptr, int32_t* dim, int64_t* stats, int32_t device);

/* ---- points in oriented boxes ---------------------------------------------------- */
/*
 * OrientedBoundingBox.get_point_indices_within_bounding_box for up to PYQSM_BOXES_MAX boxes in one pass
 * over the cloud (pyQSM's recover_original_details asks every cluster box of every tile of the scan).
 *   xyz f64 [n,3]; boxes f64 [B,15]: centre 3, R row-major 9, half-extent 3.
 *   Point p is in box k iff |t_i| <= half_i for i = 0, 1, 2, with d = p - c and
 *   t_i = (d.x * R[0][i] + d.y * R[1][i]) + d.z * R[2][i]: fp64 in exactly this order, bounds inclusive,
 *   no contraction; a NaN is in no box.
 *   ptr i64 [B + 1] (the caller's); *idx i64 [ptr[B]]: the members of box k, ascending, are
 *   idx[ptr[k]] .. idx[ptr[k + 1]]; allocated by the library, released with pyqsm_free, NULL when no
 *   point is in any box. Two passes of 24 B per point (count, scan, fill), no atomics.
 *   B > PYQSM_BOXES_MAX: PYQSM_EINVAL; n * B above 2^31 - 256: PYQSM_ERANGE (pass fewer boxes per call).
 * The _dev form takes a cloud that is already in HBM: a tile uploaded once answers any number of calls.
 */
#define PYQSM_BOXES_MAX 256
int pyqsm_points_in_boxes(const double* xyz, int64_t n, const double* boxes, int32_t B, int64_t* ptr,
                          int64_t** idx, int32_t device);
int pyqsm_points_in_boxes_dev(const double* xyz_dev, int64_t n, const double* boxes, int32_t B, int64_t* ptr,
                              int64_t** idx, int32_t device);

/* ---- colours: exact HSV classes, saturation lift, histogram, masks ---------------- */
/*
 * pyQSM's viz/color.py (segment_hues, color_distribution, saturate_colors, get_color_by_hue,
 * remove_color_pts, get_green_surfaces) on the device. All arithmetic is fp64, one operation at a time in
 * the order written here, without contraction: the conversions are matplotlib.colors.rgb_to_hsv and
 * hsv_to_rgb bit for bit (csrc/color_exact.hpp holds the one statement kernels and host share).
 *
 * rgb -> hsv, per row (r, g, b) in [0, 1]:
 *   mx = max, mn = min, d = mx - mn;  v = mx;  s = d / mx if mx > 0, else 0.
 *   If d > 0 the LAST line that holds wins:  r == mx: x = (g - b) / d;  g == mx: x = 2.0 + (b - r) / d;
 *   b == mx: x = 4.0 + (r - g) / d.  Otherwise x = 0.
 *   y = x / 6.0 (a division);  h = y + 1.0 if y < 0, else y: a tiny negative y gives h == 1.0 exactly.
 * hsv -> rgb:
 *   h6 = h * 6.0;  i = (int64) h6;  f = h6 - i;
 *   p = v * (1.0 - s);  q = v * (1.0 - (s * f));  t = v * (1.0 - (s * (1.0 - f)));
 *   (r, g, b) by i % 6: (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q); h == 1.0 gives i = 6, case 0;
 *   s == 0 gives (v, v, v).
 * Saturation lift: s' = s + (1.0 - s) / lift_div where s < min_s (strict), else s; lift_div < 1 or NaN:
 *   PYQSM_EINVAL. The corrected colour is hsv_to_rgb(h, s', v). lift_div = +inf is the identity: no lift and
 *   no round trip, the corrected colour is the input bit for bit and the class is taken on rgb_to_hsv(rgb)
 *   (pyQSM's get_color_by_hue; a round trip through hsv moves last bits even when s' == s).
 * Rules: K <= PYQSM_COLOR_MAX_RULES rows of rules f64 [K,6] = (h_lo, h_hi, s_lo, s_hi, v_lo, v_hi), ±inf for
 *   "unbounded"; closed i32 [K]: bit 2c makes the lower bound of channel c inclusive, bit 2c + 1 the upper
 *   one. A NaN bound: PYQSM_EINVAL.
 * Class: the index of the first rule that holds on rgb_to_hsv(corrected rgb) (the second conversion, after
 *   the round trip), PYQSM_COLOR_NONE when none holds.
 *
 * pyqsm_rgb_to_hsv / pyqsm_hsv_to_rgb: f64 [n,3] to f64 [n,3], host arrays.
 * pyqsm_hsv_segment: rgb f64 [n,3]; cls u8 [n]; counts i64 [K + 1] rows per class, "none" last;
 *   members i64 [n] or NULL: the CSR by class (classes 0 .. K-1, then "none"; the offsets are the running
 *   sums of counts), ascending inside a class; rgb_out / hsv_out f64 [n,3] or NULL: the corrected colours
 *   and their hsv. One pass over the rows, a scan over [class][wave], one pass over the class bytes for the
 *   members; no atomics, the same bytes on every run. n == 0 touches no device (zero counts); K == 0 is
 *   allowed (every row is "none"). n above 2^31 - 256: PYQSM_ERANGE.
 * pyqsm_hsv_segment_dev: the same with rgb, cls, members, rgb_out and hsv_out in HBM (rules, closed and
 *   counts on the host).
 * pyqsm_hsv_histogram: vals f64 [n,3], hsv rows (is_hsv != 0) or rgb rows converted first; bins i32 [3],
 *   each >= 1 (else PYQSM_EINVAL), product <= PYQSM_COLOR_MAX_BINS (else PYQSM_ERANGE). The edges of a
 *   channel with b bins are linspace(0, 1, b + 1) (j * (1.0 / b), the last one 1.0) and the bin of x is
 *   min(searchsorted(edges, x, 'right') - 1, b - 1): np.histogramdd(hsv, bins, range=[(0, 1)] * 3).
 *   which >= 0: only the rows with cls[i] == which (cls u8 [n]); which == -1: all rows, cls may be NULL.
 *   hist i64 [bins[0] * bins[1] * bins[2]], row-major. Integer atomics only.
 * pyqsm_color_mask: the ascending indices idx i64 [n] (the caller's) and their *count of the rows with
 *   PYQSM_MASK_SUM_GT: ((0.0 + r) + g) + b > param (pyQSM's "white": 2.7);
 *   PYQSM_MASK_GREEN:  g > r && g > b && 0.5 < r / b && r / b < 2 (b == 0: inf or NaN, false).
 * Input: the host forms refuse a NaN or a value outside [0, 1] with PYQSM_EINVAL before any launch (matplotlib
 *   raises there too); the _dev form raises an error word in its kernel and returns PYQSM_EINVAL after it,
 *   its outputs then unspecified.
 */
#define PYQSM_COLOR_MAX_RULES 16
#define PYQSM_COLOR_MAX_BINS 4096
#define PYQSM_COLOR_NONE 255
#define PYQSM_MASK_SUM_GT 0
#define PYQSM_MASK_GREEN 1
int pyqsm_rgb_to_hsv(const double* rgb, int64_t n, double* hsv, int32_t device);
int pyqsm_hsv_to_rgb(const double* hsv, int64_t n, double* rgb, int32_t device);
int pyqsm_hsv_segment(const double* rgb, int64_t n, double min_s, double lift_div, const double* rules,
                      const int32_t* closed, int32_t K, uint8_t* cls, int64_t* counts, int64_t* members,
                      double* rgb_out, double* hsv_out, int32_t device);
int pyqsm_hsv_segment_dev(const double* rgb_dev, int64_t n, double min_s, double lift_div, const double* rules,
                          const int32_t* closed, int32_t K, uint8_t* cls_dev, int64_t* counts,
                          int64_t* members_dev, double* rgb_out_dev, double* hsv_out_dev, int32_t device);
int pyqsm_hsv_histogram(const double* vals, int64_t n, int32_t is_hsv, const int32_t* bins, const uint8_t* cls,
                        int32_t which, int64_t* hist, int32_t device);
int pyqsm_color_mask(const double* rgb, int64_t n, int32_t kind, double param, int64_t* idx, int64_t* count,
                     int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* PYQSM_HIP_H */
