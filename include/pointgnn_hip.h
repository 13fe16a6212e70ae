/* pointgnn_hip.h -- C ABI of libpointgnn_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the hot path of WeijingShi/Point-GNN.  The reference has
 * no FFI layer (everything is Python calling TensorFlow 1.15 / scikit-learn);
 * each entry point below names the reference interface it replaces
 * (file:line relative to the reference tree).  Host code (Python, ctypes) keeps
 * the reference's operator names and only moves pointers: see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter says `host`;
 *   - the caller owns every buffer; the library never frees or retains a
 *     pointer past the call; scratch comes from a caller-provided workspace
 *     sized by the matching *_workspace_bytes() query;
 *   - every entry takes a hipStream_t (as void*) and is asynchronous with
 *     respect to the host: no hidden synchronisation.  The only process-wide
 *     mutable state is the set of diagnostic knobs behind pgnn_set_tunable /
 *     pgnn_set_debug_buffer (end of this header): launch-shape and ablation
 *     switches for benchmarks and tests whose defaults never need changing.
 *     They are plain words read once per call; change them only while no
 *     other thread is inside the library.  Everything else is re-entrant
 *     across streams and threads;
 *   - return value: 0 = ok, negative = argument error (PGNN_E_*), positive =
 *     hipError_t of the failing runtime call.  pgnn_last_error() returns a
 *     thread-local message for the last non-zero return.  No C++ exception
 *     crosses the ABI;
 *   - indices are int32 on the wire (run.py:126-133, train.py:126-128), all
 *     floating point is fp32 unless stated;
 *   - must not be called in a forked child after HIP was initialised in the
 *     parent (the reference forks graph workers, train.py:430).
 */
#ifndef POINTGNN_HIP_H_
#define POINTGNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGNN_E_INVALID (-1)   /* bad argument (null pointer, negative size...) */
#define PGNN_E_WORKSPACE (-2) /* workspace too small                          */
#define PGNN_E_UNSUPPORTED (-3) /* shape outside the implemented range        */
#define PGNN_E_CAPACITY (-4)  /* output capacity too small                    */
#define PGNN_E_COMM (-5)      /* RCCL missing / a collective call failed       */

/* ---- library ---------------------------------------------------------- */
int pgnn_version(void);
const char *pgnn_last_error(void);
/* Sanity probe used by the Python loader: 0 iff `device_ptr` is a device
 * allocation visible to the HIP runtime this library is bound to. */
int pgnn_check_device_pointer(const void *device_ptr);

/* A stream whose kernels run on CUs [cu_first, cu_first + cu_count) only, or
 * (complement != 0) on all the others.  The frame pipeline builds the next
 * frame's graph on a few reserved CUs while the fused MFMA kernels of the
 * current frame own the rest: they fill a CU completely (VGPRs and LDS), so
 * without the split a kernel of another stream waits for their kernel
 * boundaries and then displaces one of their persistent workgroups.  Mask bits
 * are striped over the XCDs (bit i -> XCD i % 8): a contiguous range takes the
 * same number of CUs from every XCD.  *stream_out is a hipStream_t; destroy it
 * with pgnn_stream_destroy.  Every other entry takes such a stream like any
 * other. */
int pgnn_stream_create_cu_mask(int32_t cu_first, int32_t cu_count,
                               int32_t complement, void **stream_out);
int pgnn_stream_destroy(void *stream);

/* ---- scatter-max -------------------------------------------------------
 * Replaces graph_scatter_max_fn = tf.math.unsorted_segment_max
 * (models/gnn.py:106-109; call sites gnn.py:275-277, 362-365).
 * out[s, c] = max over rows r with seg_ids[r] == s of data[r, c]; a segment
 * with no rows gets the lowest finite float (TF semantics).  Ids outside
 * [0, num_segments) are ignored.  `ids_sorted` != 0 promises that seg_ids is
 * non-decreasing (what the radius-graph builder emits): whole-segment runs
 * are then written with plain stores instead of atomics.  Any order is
 * accepted when ids_sorted == 0.  ld_* are row strides in floats; pad columns
 * of `out` (ld_out > n_cols) are left untouched.
 * One result, one bit pattern: every cell is max(lowest, its rows) + 0.0f,
 * i.e. TF's initialise-with-lowest-then-max with a zero written as +0.0.  A
 * segment of only -0.0 gives +0.0 and a segment of only -inf gives the lowest
 * finite float, whatever ids_sorted, the tunables or the device make of the
 * row ranges (plain stores and atomics write the same form).  NaN rows are
 * unspecified, as in TF.  n_cols <= 2048 when n_cols and both strides are
 * multiples of 4 and both pointers 16-byte aligned, <= 1024 otherwise
 * (PGNN_E_UNSUPPORTED beyond).
 * Algorithmic bytes: n_rows*n_cols*4 + n_rows*4 + num_segments*n_cols*4. */
int pgnn_scatter_max_f32(const float *data, int64_t ld_data,
                         const int32_t *seg_ids, int64_t n_rows,
                         int32_t n_cols, int32_t num_segments, float *out,
                         int64_t ld_out, int32_t ids_sorted, void *stream);

/* graph_scatter_sum_fn / graph_scatter_mean_fn = tf.math.unsorted_segment_sum /
 * unsorted_segment_mean (models/gnn.py:111-119; registered by the reference,
 * used by no shipped config).  Same arguments as pgnn_scatter_max_f32; `mean`
 * != 0 divides every segment by max(count, 1) (empty segments give 0, as in
 * TF) and needs `counts_ws`, int32[num_segments] of scratch.  Float atomic
 * adds: the summation order is unspecified, as on TensorFlow's GPU kernel. */
int pgnn_scatter_sum_f32(const float *data, int64_t ld_data,
                         const int32_t *seg_ids, int64_t n_rows, int32_t n_cols,
                         int32_t num_segments, float *out, int64_t ld_out,
                         int32_t mean, int32_t *counts_ws, void *stream);

/* ---- radius graph ------------------------------------------------------
 * Replaces gen_disjointed_rnn_local_graph_v3 (models/graph_gen.py:197-220):
 * for every centre, all points with float64 squared distance <= radius^2
 * (inclusive; scikit-learn ball-tree semantics).  Two phases, no hidden
 * sync:  count -> caller reads offsets[n_centers] and allocates -> fill.
 * `scale3` (host pointer to 3 doubles, may be NULL) is the reference's
 * optional `scale` pre-division (graph_gen.py:203-206).
 * Output rows are (point_idx, centre_idx), grouped by ascending centre.  */
size_t pgnn_radius_graph_workspace_bytes(int64_t n_points, int64_t n_centers);
int pgnn_radius_graph_count(const float *points, int64_t n_points,
                            const float *centers, int64_t n_centers,
                            double radius, const double *scale3_host,
                            void *workspace, size_t workspace_bytes,
                            int32_t *offsets /* [n_centers + 1] */,
                            void *stream);
int pgnn_radius_graph_fill(const float *points, int64_t n_points,
                           const float *centers, int64_t n_centers,
                           double radius, const double *scale3_host,
                           void *workspace, size_t workspace_bytes,
                           const int32_t *offsets /* from _count */,
                           int32_t *edges /* [capacity, 2] */,
                           int64_t capacity, void *stream);
/* The same two phases on FLOAT64 points / centres: the training data path
 * keeps the augmented cloud float64 through graph generation (train.py:88-90
 * -> graph_gen.py:187-194; the cast to float32 is train.py:124), and sklearn
 * searches float64 data as it is.  Same workspace query, same outputs. */
int pgnn_radius_graph_count_f64(const double *points, int64_t n_points,
                                const double *centers, int64_t n_centers,
                                double radius, const double *scale3_host,
                                void *workspace, size_t workspace_bytes,
                                int32_t *offsets /* [n_centers + 1] */,
                                void *stream);
int pgnn_radius_graph_fill_f64(const double *points, int64_t n_points,
                               const double *centers, int64_t n_centers,
                               double radius, const double *scale3_host,
                               void *workspace, size_t workspace_bytes,
                               const int32_t *offsets /* from _count */,
                               int32_t *edges /* [capacity, 2] */,
                               int64_t capacity, void *stream);
/* ---- k nearest neighbours within the radius (extension) -----------------
 * An EXTENSION of gen_disjointed_rnn_local_graph_v3 (models/graph_gen.py:
 * 197-220): the reference bounds a neighbourhood with np.random.choice only
 * (its neighbors_downsample_method hook ignores every value but 'random');
 * these entries keep the k nearest points of the radius neighbourhood.
 * Inputs as pgnn_radius_graph_count / _fill: points [n_points, 3] and centres
 * [n_centers, 3], both float32 or (_f64) both float64, radius > 0, optional
 * scale3_host; new: k, 1 <= k <= 256 (256 is the num_neighbors of the shipped
 * training configs).  k > 256 returns PGNN_E_UNSUPPORTED; k < 1 returns
 * PGNN_E_INVALID before any HIP call.  For every centre q:
 *   Candidate set: N(q) is exactly the set of points the radius graph returns
 *     for q, by the same arithmetic: coordinates pre-divided by scale3,
 *     d2 = (dx*dx + dy*dy) + dz*dz in float64 with no contraction, and
 *     d2 <= r*r, inclusive.
 *   Selection: the min(k, |N(q)|) members of N(q) with the smallest key
 *     (d2, point index), compared lexicographically -- equal distances are
 *     broken by the smaller point index, so duplicate points and lattice ties
 *     are defined.
 *   Rows: (point_idx, centre_idx), grouped by ascending centre and sorted by
 *     ascending key inside a centre; offsets[n_centers + 1] is the CSR of the
 *     groups.  Hence offsets[q+1] - offsets[q] == min(k, radius fan-in of q)
 *     and the rows of a centre are a subset of its radius-graph rows.  The
 *     order is independent of the cell grid (the radius graph's own row order
 *     is not part of this contract).
 *   NaN coordinates: unspecified, as in the radius graph.
 * Two phases, no hidden sync: count -> caller reads offsets[n_centers] and
 * allocates -> fill (same workspace, same arguments).  Rows at or beyond
 * `capacity` are not written, as in pgnn_radius_graph_fill.  The uncapped
 * neighbour list is never materialised: the workspace is a function of
 * (n_points, n_centers, k) alone (0 for an unsupported k). */
size_t pgnn_knn_graph_workspace_bytes(int64_t n_points, int64_t n_centers,
                                      int32_t k);
int pgnn_knn_graph_count(const float *points, int64_t n_points,
                         const float *centers, int64_t n_centers,
                         double radius, const double *scale3_host, int32_t k,
                         void *workspace, size_t workspace_bytes,
                         int32_t *offsets /* [n_centers + 1] */,
                         void *stream);
int pgnn_knn_graph_fill(const float *points, int64_t n_points,
                        const float *centers, int64_t n_centers,
                        double radius, const double *scale3_host, int32_t k,
                        void *workspace, size_t workspace_bytes,
                        const int32_t *offsets /* from _count */,
                        int32_t *edges /* [capacity, 2] */,
                        int64_t capacity, void *stream);
/* float64 points / centres (extension of models/graph_gen.py:197-220 on the
 * training path's float64 cloud, like pgnn_radius_graph_count_f64). */
int pgnn_knn_graph_count_f64(const double *points, int64_t n_points,
                             const double *centers, int64_t n_centers,
                             double radius, const double *scale3_host,
                             int32_t k, void *workspace,
                             size_t workspace_bytes,
                             int32_t *offsets /* [n_centers + 1] */,
                             void *stream);
int pgnn_knn_graph_fill_f64(const double *points, int64_t n_points,
                            const double *centers, int64_t n_centers,
                            double radius, const double *scale3_host,
                            int32_t k, void *workspace, size_t workspace_bytes,
                            const int32_t *offsets /* from _count */,
                            int32_t *edges /* [capacity, 2] */,
                            int64_t capacity, void *stream);
/* Capacity form of the same builder -- count, scan and fill in ONE call with
 * no size leaving the device (graph_gen.py:155-220 never waits for one: its
 * NumPy arrays carry their sizes; a device pipeline that reads K or E back
 * stalls the host once per level).  `points_cap` / `centers_cap` size the
 * launches and the workspace; when `n_points_dev` / `n_centers_dev` (device
 * int32, nullable) are given, min(*n_dev, cap) rows are valid -- this is how a
 * level takes the keypoints of pgnn_voxel_keypoints_* (whose count is
 * num_keypoints[0] on the device) as its points and centres.  Rows are written
 * up to `edge_capacity`; n_edges_dev[0] = rows written = min(E, capacity),
 * n_edges_dev[1] = E, the size required: the caller compares the two when it
 * reads the frame's results and re-runs with a larger buffer if they differ.
 * Same rows, same order as _count + _fill. */
size_t pgnn_radius_graph_dyn_workspace_bytes(int64_t points_cap,
                                             int64_t centers_cap);
int pgnn_radius_graph_dyn(const float *points, int64_t points_cap,
                          const int32_t *n_points_dev, const float *centers,
                          int64_t centers_cap, const int32_t *n_centers_dev,
                          double radius, const double *scale3_host,
                          void *workspace, size_t workspace_bytes,
                          int32_t *edges /* [edge_capacity, 2] */,
                          int64_t edge_capacity,
                          int32_t *n_edges_dev /* [2], device */, void *stream);
int pgnn_radius_graph_dyn_f64(const double *points, int64_t points_cap,
                              const int32_t *n_points_dev,
                              const double *centers, int64_t centers_cap,
                              const int32_t *n_centers_dev, double radius,
                              const double *scale3_host, void *workspace,
                              size_t workspace_bytes, int32_t *edges,
                              int64_t edge_capacity, int32_t *n_edges_dev,
                              void *stream);
/* The same builder in its two stages, for a caller that overlaps them with
 * other work: _grid needs the points only (cell keys, radix sort, bucket
 * bounds), _query the centres as well (count, scan, fill).  A frame's level-0
 * graph has the raw cloud as its points and the keypoints as its centres, so
 * its grid stage can run on a second stream BESIDE the keypoint selection and
 * only the query stage has to wait for it (the caller orders the two with its
 * own stream / event calls; both stages take the SAME workspace, capacities,
 * radius and scale).  _grid then _query on one stream is pgnn_radius_graph_dyn
 * exactly. */
int pgnn_radius_graph_dyn_grid(const float *points, int64_t points_cap,
                               const int32_t *n_points_dev, int64_t centers_cap,
                               double radius, const double *scale3_host,
                               void *workspace, size_t workspace_bytes,
                               void *stream);
int pgnn_radius_graph_dyn_grid_f64(const double *points, int64_t points_cap,
                                   const int32_t *n_points_dev,
                                   int64_t centers_cap, double radius,
                                   const double *scale3_host, void *workspace,
                                   size_t workspace_bytes, void *stream);
int pgnn_radius_graph_dyn_query(const float *points, int64_t points_cap,
                                const float *centers, int64_t centers_cap,
                                const int32_t *n_centers_dev, double radius,
                                const double *scale3_host, void *workspace,
                                size_t workspace_bytes, int32_t *edges,
                                int64_t edge_capacity, int32_t *n_edges_dev,
                                void *stream);
int pgnn_radius_graph_dyn_query_f64(const double *points, int64_t points_cap,
                                    const double *centers, int64_t centers_cap,
                                    const int32_t *n_centers_dev, double radius,
                                    const double *scale3_host, void *workspace,
                                    size_t workspace_bytes, int32_t *edges,
                                    int64_t edge_capacity, int32_t *n_edges_dev,
                                    void *stream);
/* Training-time fan-in cap (graph_gen.py:210-214, num_neighbors > 0): keeps a
 * uniformly random subset (without replacement) of `max_neighbors` edges for
 * every centre whose fan-in exceeds it (counter-based RNG keyed by `seed`,
 * centre and position).  Two phases like the builder: _count writes
 * new_offsets[n_centers + 1] from the uncapped CSR offsets; the caller reads
 * the total and allocates; _fill writes the surviving rows, same grouping. */
int pgnn_cap_neighbors_count(const int32_t *offsets, int64_t n_centers,
                             int32_t max_neighbors, int32_t *new_offsets,
                             void *stream);
int pgnn_cap_neighbors_fill(const int32_t *offsets, const int32_t *edges,
                            int64_t n_centers, int32_t max_neighbors,
                            uint64_t seed, const int32_t *new_offsets,
                            int32_t *new_edges, int64_t new_capacity,
                            void *stream);
/* The cap in capacity form (no host read), for a level built by
 * pgnn_radius_graph_dyn(_query)(_f64): takes that call's workspace (the CSR
 * offsets it left there; same points_cap / centers_cap), its edge rows and its
 * record n_edges_dev[2]; writes new_offsets[centers_cap + 1], the surviving
 * rows (same rows, same order as _count + _fill with this seed) up to
 * `new_capacity`, and the capped list's record n_new_dev[2] = {rows written,
 * rows required}.  If the UNCAPPED list overflowed its own capacity the capped
 * record reads {0, required}: the level is flagged the usual way (required >
 * written) and the caller rebuilds it. */
int pgnn_radius_graph_dyn_cap(const void *workspace, size_t workspace_bytes,
                              int64_t points_cap, int64_t centers_cap,
                              const int32_t *edges, int64_t edge_capacity,
                              const int32_t *n_edges_dev /* [2], device */,
                              int32_t max_neighbors, uint64_t seed,
                              int32_t *new_offsets, int32_t *new_edges,
                              int64_t new_capacity,
                              int32_t *n_new_dev /* [2], device */,
                              void *stream);
/* ---- k nearest neighbours without a radius (extension) ------------------
 * The third neighbourhood of a point-cloud GNN beside the radius graph and the
 * kNN within a radius above: the k nearest points of the WHOLE cloud, so every
 * centre has the same fan-in whatever the local density.  Inputs: points
 * [points_cap, 3] and centres [centers_cap, 3], both float32 or (_f64) both
 * float64, optional scale3_host, 1 <= k <= 256, cell_size > 0.  k < 1 or
 * cell_size <= 0 returns PGNN_E_INVALID before any HIP call; k > 256 returns
 * PGNN_E_UNSUPPORTED.  For every centre q:
 *   Coordinates and distance: widened to float64 and pre-divided by scale3;
 *     d2 = (dx*dx + dy*dy) + dz*dz in float64 with no contraction -- the
 *     arithmetic of the radius graph and of pgnn_knn_graph_*.
 *   Selection: the m = min(k, number of points) points with the smallest key
 *     (d2, point index), compared lexicographically, so duplicate points and
 *     lattice ties are defined.
 *   Rows: (point_idx, centre_idx); centre q owns rows [q*m, (q+1)*m), in
 *     ascending key order.  There is no offsets array: the CSR is arithmetic
 *     and E = centres * m.  When points and centres are the same array the
 *     centre itself is a candidate (d2 = 0), as in the radius graph.
 *   cell_size: the edge of the search grid, in scaled units.  It is a tuning
 *     argument ONLY: the rows are a function of (points, centres, scale, k) and
 *     never of cell_size.  (It must keep |coordinate / cell_size| below 2^29;
 *     a good value holds a few times k points per 27 cells.)
 *   NaN coordinates: unspecified, as in the radius graph.
 * One call, no host read, in the style of pgnn_radius_graph_dyn: with both
 * n_points_dev and n_centers_dev NULL the caps ARE the sizes (host-sized form,
 * E = centers_cap * min(k, points_cap) is known to the caller); when given
 * (device int32), min(*n_dev, cap) rows are valid and m = min(k, valid points)
 * is evaluated on the device.  n_edges_dev (nullable) receives {rows written,
 * rows required} = {min(E, edge_capacity), E}; rows at or beyond edge_capacity
 * are not written.  Zero valid points or zero valid centres give {0, 0} and
 * write nothing.  centers_cap * k must fit an int32.  The workspace is a
 * function of (points_cap, centers_cap, k) alone (0 for an unsupported k). */
size_t pgnn_knn_nearest_workspace_bytes(int64_t points_cap,
                                        int64_t centers_cap, int32_t k);
int pgnn_knn_nearest(const float *points, int64_t points_cap,
                     const int32_t *n_points_dev, const float *centers,
                     int64_t centers_cap, const int32_t *n_centers_dev,
                     const double *scale3_host, int32_t k, double cell_size,
                     void *workspace, size_t workspace_bytes,
                     int32_t *edges /* [edge_capacity, 2] */,
                     int64_t edge_capacity,
                     int32_t *n_edges_dev /* [2], device, nullable */,
                     void *stream);
int pgnn_knn_nearest_f64(const double *points, int64_t points_cap,
                         const int32_t *n_points_dev, const double *centers,
                         int64_t centers_cap, const int32_t *n_centers_dev,
                         const double *scale3_host, int32_t k,
                         double cell_size, void *workspace,
                         size_t workspace_bytes, int32_t *edges,
                         int64_t edge_capacity, int32_t *n_edges_dev,
                         void *stream);

/* ---- keypoints ----------------------------------------------------------
 * 'center' mode = multi_layer_downsampling_select (graph_gen.py:49-90) for ONE
 * pooling level per call (the reference loops over arbitrary `levels`; every
 * shipped config has one downsampling level followed by equal scales, which
 * graph_gen.py:76-81 turns into copies.  These entries serve the FIRST
 * pooling level -- the search set is the voxelised cloud itself; the levels
 * above it take pgnn_voxel_keypoints_*_from below, and the Python mirror
 * pointgnn_amd.graph_gen loops over the levels like the reference):
 * open3d-0.7 voxel centroids (origin = min_bound - voxel/2,
 * float64 means in point order) followed by an exact float64 1-NN back to a
 * real point; exact distance ties are broken like scikit-learn's kd-tree
 * query does (see pgnn_kdtree_replica).  Keypoints are emitted in ascending
 * voxel-hash order.
 * 'random' mode = multi_layer_downsampling_random (graph_gen.py:92-153): one
 * uniformly chosen point per occupied voxel of the grid anchored at the
 * cloud minimum (+ `jitter3_host`, the reference's add_rnd3d origin shift,
 * in units of metres; NULL = none), RNG keyed by `seed`.
 * Capacity of both outputs is n_points rows.  num_keypoints: device int32[2],
 * [0] = K, [1] = tie-order status of the kd-tree replica ('center' only; 0 =
 * the reference's order -- libstdc++'s introselect INCLUDING its heap-select
 * fallback is replayed; non-zero = the cloud is outside what the replica
 * reproduces, exact 1-NN ties may then be broken differently from the
 * reference; the Python mirror raises on it).
 * Limits of 'center' mode: float32 points only (the replica's keys), at most
 * 524 288 points (PGNN_E_UNSUPPORTED beyond: node records are kept in LDS).
 * The tie rule replicated is scikit-learn >= 1.0's (std::nth_element in
 * sklearn/neighbors/_partition_nodes.pyx); the reference pins no version and a
 * 2020-era 0.22 partitions differently.                                     */
/* Replica of scikit-learn's KDTree(points, leaf_size=30) node order -- what
 * decides which of several exactly equidistant points
 * NearestNeighbors(algorithm='kd_tree').kneighbors returns (graph_gen.py:84-88)
 * and therefore the reference's keypoint in every 2-point voxel.
 * pgnn_voxel_keypoints_center builds it internally; this entry exposes the
 * arrays (device pointers) for tests against KDTree.get_arrays():
 *   idx_array   [n_points]      int32   (sklearn: intp)
 *   node_bounds [n_nodes][6]    float64 (lo x,y,z, hi x,y,z; sklearn stores
 *                                        [2][n_nodes][3])
 *   status      [1]             int32   0, or 1 if std::nth_element's
 *                                        heap-select fallback would have been
 *                                        taken (not replicated)
 * pgnn_kdtree_shape returns sklearn's n_levels / n_nodes for n_points (host
 * pointers).                                                              */
int pgnn_kdtree_shape(int64_t n_points, int32_t *n_levels, int32_t *n_nodes);
size_t pgnn_kdtree_workspace_bytes(int64_t n_points);
int pgnn_kdtree_replica(const float *points, int64_t n_points, void *workspace,
                        size_t workspace_bytes, int32_t *idx_array,
                        double *node_bounds, int32_t *status, void *stream);

size_t pgnn_keypoints_workspace_bytes(int64_t n_points);  /* either precision */
/* aux_stream (nullable): a second caller-owned stream.  When given, the
 * kd-tree replica (a latency-bound chain of ~10 dependent launches that only
 * needs the points) is issued there, forked from and joined back into `stream`
 * with two events, so it overlaps the voxel hashing; NULL = everything in
 * order on `stream`.  The results are identical. */
int pgnn_voxel_keypoints_center(const float *points, int64_t n_points,
                                double voxel_size, void *workspace,
                                size_t workspace_bytes,
                                int32_t *keypoint_indices, float *keypoint_xyz,
                                int32_t *num_keypoints, void *stream,
                                void *aux_stream);
int pgnn_voxel_keypoints_random(const float *points, int64_t n_points,
                                double voxel_size, const double *jitter3_host,
                                uint64_t seed, void *workspace,
                                size_t workspace_bytes,
                                int32_t *keypoint_indices, float *keypoint_xyz,
                                int32_t *num_keypoints, void *stream);

/* 'random' mode on a FLOAT64 cloud (train.py:88-90): NumPy's float64 `//` on
 * (points - min) [+ jitter] (graph_gen.py:123-128); keypoint_xyz is float64
 * (the reference returns rows of its float64 array).  */
int pgnn_voxel_keypoints_random_f64(const double *points, int64_t n_points,
                                    double voxel_size,
                                    const double *jitter3_host, uint64_t seed,
                                    void *workspace, size_t workspace_bytes,
                                    int32_t *keypoint_indices,
                                    double *keypoint_xyz,
                                    int32_t *num_keypoints, void *stream);

/* The second and later POOLING levels of a frame (graph_gen.py:49-90 and
 * :92-153 loop over arbitrary `levels`; every shipped config has one pooling
 * level, which the entries above serve):
 *   'center' (graph_gen.py:41-45, :78-88): the centroids are still those of
 *     the ORIGINAL cloud's voxels (`points`, at this level's voxel size), but
 *     the 1-NN search runs among `search_points` = the previous level's
 *     keypoint coordinates, with scikit-learn's kd-tree order over THAT set
 *     deciding exact ties.  keypoint_indices index search_points;
 *     keypoint_xyz = search_points[keypoint_indices].  num_keypoints as above
 *     ([1] = the tie-order status of the kd-tree replica of search_points).
 *   'random' (graph_gen.py:108-110, :121-150): `points` = the previous level's
 *     keypoints are voxelised on the grid anchored at the minimum of
 *     `origin_points` = the ORIGINAL cloud (n_origin = 0: of `points`).
 * Workspace: pgnn_keypoints_from_workspace_bytes(n_points, n_search) for
 * 'center', pgnn_keypoints_workspace_bytes(n_points) for 'random'.            */
size_t pgnn_keypoints_from_workspace_bytes(int64_t n_points, int64_t n_search);
int pgnn_voxel_keypoints_center_from(const float *points, int64_t n_points,
                                     const float *search_points,
                                     int64_t n_search, double voxel_size,
                                     void *workspace, size_t workspace_bytes,
                                     int32_t *keypoint_indices,
                                     float *keypoint_xyz,
                                     int32_t *num_keypoints, void *stream);
int pgnn_voxel_keypoints_random_from(const float *points, int64_t n_points,
                                     const float *origin_points,
                                     int64_t n_origin, double voxel_size,
                                     const double *jitter3_host, uint64_t seed,
                                     void *workspace, size_t workspace_bytes,
                                     int32_t *keypoint_indices,
                                     float *keypoint_xyz,
                                     int32_t *num_keypoints, void *stream);
int pgnn_voxel_keypoints_random_from_f64(
    const double *points, int64_t n_points, const double *origin_points,
    int64_t n_origin, double voxel_size, const double *jitter3_host,
    uint64_t seed, void *workspace, size_t workspace_bytes,
    int32_t *keypoint_indices, double *keypoint_xyz, int32_t *num_keypoints,
    void *stream);

/* ---- dense layers --------------------------------------------------------
 * A fully connected layer y = act(x @ W + b) (slim.fully_connected with
 * normalizer 'NONE', models/gnn.py:86-104 and :34-84) is held on the device in
 * MFMA-fragment order: pgnn_pack_fc() converts the reference's [k_in, n_out]
 * row-major weights + bias (HOST pointers) into `packed` (HOST, then copied to
 * the device by the caller).  Layout: kq = ceil(k_in/16) K-groups, nt =
 * ceil(n_out/16) column tiles; packed[((q*nt + t)*64 + lane)*4 + s] =
 * W[16q + 4*(lane>>4) + s][16t + (lane&15)] (zero outside), followed by
 * bias[16*nt] (zero padded).                                               */
size_t pgnn_packed_fc_floats(int32_t k_in, int32_t n_out);
int pgnn_pack_fc(const float *w_host, const float *b_host, int32_t k_in,
                 int32_t n_out, float *packed_host);

typedef struct pgnn_fc_layer {
  const float *packed; /* device: pgnn_pack_fc image                         */
  int32_t k_in;        /* logical input width (<= 16*kq)                     */
  int32_t n_out;       /* logical output width                               */
  int32_t relu_from;   /* ReLU on output columns >= relu_from; 0 = every
                          column, >= n_out = linear layer (is_logits)        */
} pgnn_fc_layer;

#define PGNN_MAX_LAYERS 8

/* ---- capacity form of the per-frame operators ------------------------------
 * The reference's graph builder hands NumPy arrays to the model
 * (run.py:219-222 -> 245-260): sizes travel with the arrays and nobody waits
 * for them.  On the device the keypoint count K and the edge counts exist
 * only after the builder's kernels ran; reading them back to size the next
 * launch stalls the host twice per frame.  The *_dyn entries below are the
 * operators of this section with every such count taken from DEVICE memory:
 * the ordinary size argument becomes the capacity (it sizes buffers and
 * grids), `dev` points at the int32 count (min(*dev, capacity) rows are
 * processed; the rows behind it are neither read nor written), and `hint` is
 * the count the host expects (e.g. the previous frame's): it only chooses
 * between kernels that give bit-identical results (weights-stationary vs
 * LDS-tile, 8-wave vs 4-wave rows kernel) and sizes strided grids, so a wrong
 * hint costs time, never correctness.  hint <= 0 means the capacity. */
typedef struct pgnn_dyn_count {
  const int32_t *dev; /* device int32: the actual count                     */
  int64_t hint;       /* expected value (host), <= 0: unknown               */
} pgnn_dyn_count;

/* Per-row MLP chain: y = MLP(concat(x[:, :nx], x2[:, :nx2])) (+ residual).
 * Covers multi_layer_neural_network_fn / multi_layer_fc_fn on per-vertex
 * inputs: PointSetPooling's output MLP (gnn.py:279-282), the auto-offset MLP
 * (gnn.py:341-346), the update MLP + residual (gnn.py:367-372) and, with a
 * block-diagonal packing, ClassAwarePredictor (gnn.py:133-163).  x2 / residual
 * may be NULL.  y receives 16*ceil(n_out_last/16) columns per row (zero
 * padded), so ld_y must be >= that.                                         */
int pgnn_mlp_fwd(const float *x, int64_t ld_x, int32_t nx, const float *x2,
                 int64_t ld_x2, int32_t nx2, int64_t n_rows,
                 const pgnn_fc_layer *layers_host, int32_t n_layers,
                 const float *residual, int64_t ld_res, float *y, int64_t ld_y,
                 void *stream);
int pgnn_mlp_fwd_dyn(const float *x, int64_t ld_x, int32_t nx, const float *x2,
                     int64_t ld_x2, int32_t nx2, int64_t rows_cap,
                     const pgnn_fc_layer *layers_host, int32_t n_layers,
                     const float *residual, int64_t ld_res, float *y,
                     int64_t ld_y, const pgnn_dyn_count *n_rows, void *stream);

/* Fused PointSetPooling front half (gnn.py:256-277): for every edge
 * (point, keypoint) build [features(point), xyz(point) - xyz(keypoint)], run
 * the point MLP (every layer ReLU) and scatter-max into the keypoint row.
 * Nothing of size E x C touches HBM.  `edges` must be grouped by ascending
 * keypoint when edges_sorted != 0.  out: [num_keypoints, ld_out], columns
 * 16*ceil(n_out/16) written (zero padded); keypoints without edges get
 * float lowest (TF unsorted_segment_max).                                   */
/* sched_ws (both fused entries; nullable): PGNN_SCHED_WS_INTS int32 on the
 * device, zero before the first use; the kernels leave them zero.  When given,
 * the last part of the row tiles (~12-15 %) is not part of the workgroups' /
 * waves' fixed ranges but a pool they take a tile or a small chunk at a time
 * through atomic counters when their own range is done: slack that absorbs
 * uneven ranges and a late start of some workgroups (kernels of other streams
 * occupying CUs when the grid starts).  Launches that may run concurrently
 * (different streams) need different sched_ws.  Results do not depend on it
 * (max is exact). */
#define PGNN_SCHED_WS_INTS 64
int pgnn_point_set_pooling_fwd(const float *point_features, int32_t n_feat,
                               const float *point_xyz,
                               const int32_t *keypoint_indices,
                               const int32_t *edges, int64_t n_edges,
                               int32_t num_keypoints,
                               const pgnn_fc_layer *layers_host,
                               int32_t n_layers, int32_t edges_sorted,
                               float *out, int64_t ld_out, int32_t *sched_ws,
                               void *stream);
int pgnn_point_set_pooling_fwd_dyn(const float *point_features, int32_t n_feat,
                                   const float *point_xyz,
                                   const int32_t *keypoint_indices,
                                   const int32_t *edges, int64_t edges_cap,
                                   int32_t keypoints_cap,
                                   const pgnn_fc_layer *layers_host,
                                   int32_t n_layers, int32_t edges_sorted,
                                   float *out, int64_t ld_out,
                                   int32_t *sched_ws,
                                   const pgnn_dyn_count *n_edges,
                                   const pgnn_dyn_count *num_keypoints,
                                   void *stream);

/* The same with a caller-provided workspace (gnn.py:256-277; the reference
 * materialises every layer's [E, C] tensor, this entry at most one of them).
 * Point MLPs whose last layer does not fit one CU's LDS -- ped_cyl's
 * 4-32-64-128-256-512 (configs/ped_cyl_auto_T3_trainval_config) -- run as TWO
 * launches: the chain up to the 256-wide hidden layer, its rows written to
 * `workspace` ([edges_cap, 256] floats), then the last layer weights-stationary
 * in four column groups with the segmented max (csrc/pool_split.h): 0.85 of
 * the fp32-MFMA peak against the one-launch LDS-tile kernel's 0.67, the maxima
 * bit-identical.  pgnn_point_set_pooling_workspace_bytes says how much
 * workspace a chain / edge count asks for (0: the one-launch kernels are used
 * and `workspace` may be NULL; edges_hint as pgnn_dyn_count.hint, 0 = none).
 * n_edges / num_keypoints: both NULL (host-sized form: edges_cap and
 * keypoints_cap are the counts) or both given (capacity form).  `workspace`:
 * 16-byte aligned, owned by the caller, free for reuse once the call's work on
 * `stream` is done (too small: PGNN_E_WORKSPACE, nothing launched); NULL or a
 * chain the split form does not cover: exactly pgnn_point_set_pooling_fwd(_dyn). */
int pgnn_point_set_pooling_workspace_bytes(const pgnn_fc_layer *layers_host,
                                           int32_t n_layers, int32_t n_feat,
                                           int64_t edges_cap,
                                           int64_t edges_hint, size_t *bytes);
int pgnn_point_set_pooling_fwd_ws(const float *point_features, int32_t n_feat,
                                  const float *point_xyz,
                                  const int32_t *keypoint_indices,
                                  const int32_t *edges, int64_t edges_cap,
                                  int32_t keypoints_cap,
                                  const pgnn_fc_layer *layers_host,
                                  int32_t n_layers, int32_t edges_sorted,
                                  float *out, int64_t ld_out, int32_t *sched_ws,
                                  const pgnn_dyn_count *n_edges,
                                  const pgnn_dyn_count *num_keypoints,
                                  void *workspace, size_t workspace_bytes,
                                  void *stream);

/* Training forward of the same: the fused kernel also writes the point MLP's
 * activations -- acts_host[0..3] (a HOST array of four DEVICE pointers):
 * [n_edges, 32], [n_edges, 64], [n_edges, 128] and [n_edges, ld_last] for the
 * shipped car chain 4-32-64-128-300 -- which the backward needs (the last one
 * against `out` gives the arg-max rows: rows and maxima come from the same
 * accumulators).  PGNN_E_UNSUPPORTED, having done nothing, for other chains
 * or fewer than ~65k edges: run pgnn_pool_features_fwd + pgnn_mlp_fwd per
 * layer + pgnn_scatter_max_f32 instead.  edges_sorted: bit 0 = grouped by
 * ascending dst; bit 1 = `out` already holds lowest() (the native trainer
 * fills it in the launch before: no fill launch inside the call); the same
 * two bits on pgnn_edge_mlp_scatter_max_rows_fwd.                            */
int pgnn_point_set_pooling_rows_fwd(const float *point_features, int32_t n_feat,
                                    const float *point_xyz,
                                    const int32_t *keypoint_indices,
                                    const int32_t *edges, int64_t n_edges,
                                    int32_t num_keypoints,
                                    const pgnn_fc_layer *layers_host,
                                    int32_t n_layers, int32_t edges_sorted,
                                    float *out, int64_t ld_out,
                                    float *const *acts_host, int64_t ld_last,
                                    void *stream);

/* Fused GraphNetAutoCenter edge stage (gnn.py:338-365).  The first edge layer
 * is linear before its ReLU, so with P = [h, x] @ W1 + b1 and Q = x' @ W1[C:]
 * (both per vertex, computed by pgnn_mlp_fwd / pgnn_offset_apply) the
 * per-edge hidden vector is ReLU(P[src] - Q[dst]); this entry gathers it,
 * applies the remaining edge layers (ReLU) and scatter-maxes into dst rows.
 * P, Q: [num_vertices, ld_pq] with ld_pq = 16*ceil(width/16), zero padded.
 * edges_sorted: bit 0 = edges sorted by dst; bit 1 = `out` already holds
 * float lowest() everywhere (pgnn_vertex_pre_edge_fwd filled it), skip the
 * fill.                                                                      */
int pgnn_edge_mlp_scatter_max_fwd(const float *P, const float *Q,
                                  int64_t ld_pq, int32_t width,
                                  const int32_t *edges, int64_t n_edges,
                                  int32_t num_vertices,
                                  const pgnn_fc_layer *layers_host,
                                  int32_t n_layers, int32_t edges_sorted,
                                  float *out, int64_t ld_out, int32_t *sched_ws,
                                  void *stream);
int pgnn_edge_mlp_scatter_max_fwd_dyn(const float *P, const float *Q,
                                      int64_t ld_pq, int32_t width,
                                      const int32_t *edges, int64_t edges_cap,
                                      int32_t vertices_cap,
                                      const pgnn_fc_layer *layers_host,
                                      int32_t n_layers, int32_t edges_sorted,
                                      float *out, int64_t ld_out,
                                      int32_t *sched_ws,
                                      const pgnn_dyn_count *n_edges,
                                      const pgnn_dyn_count *num_vertices,
                                      void *stream);

/* ---- sum / mean aggregation of the two fused stages ----------------------
 * The reference injects the aggregator into both operators (gnn.py:211-220,
 * 285-296) and ships three: graph_scatter_max_fn, graph_scatter_sum_fn and
 * graph_scatter_mean_fn (gnn.py:106-119).  The four *_agg_* entries below are
 * the entries above with the aggregator as an argument:
 *   PGNN_AGG_MAX   exactly the entry above (workspace not read);
 *   PGNN_AGG_SUM   tf.math.unsorted_segment_sum of the per-edge rows
 *                  act(h W + b): a segment without edges gives a row of zeros,
 *                  ids outside [0, K) contribute nothing, pad columns are 0;
 *   PGNN_AGG_MEAN  tf.math.unsorted_segment_mean: the sum, then every row
 *                  divided by max(in-degree, 1) in one finishing pass (the
 *                  in-degrees: one pass over the dst column, integer atomics);
 *   anything else  PGNN_E_INVALID.
 * Sum and mean zero `out` themselves (bit 1 of edges_sorted is ignored) and
 * run the weights-stationary kernels with the sum epilogue (csrc/ws_sum.h)
 * where the max entries run theirs: one 300x300 / 256x256 edge layer, car's
 * 4-32-64-128-300 point MLP, ~65k edges and more.  Bias and ReLU are applied
 * to every edge row before it is added (they do not commute with a sum).
 * Whole segments are stored, segments that span two waves' ranges or belong to
 * an unsorted list are added with float atomics: their last bits may differ
 * from run to run, as with TensorFlow's kernel.  Anywhere else the host-sized
 * entries compose the stage from pgnn_edge_hidden_fwd / pgnn_pool_features_fwd,
 * pgnn_mlp_fwd and pgnn_scatter_sum_f32 with the per-edge rows in `workspace`;
 * the _dyn entries return PGNN_E_UNSUPPORTED there, having enqueued nothing.
 * `workspace`: device memory, 16-byte aligned, owned by the caller, free for
 * reuse once the call's work on `stream` is done; the *_agg_workspace_bytes
 * query says how much a call takes (the in-degrees for a mean, the rows of the
 * composed path; 0: may be NULL) for the stream it will run on --
 * capacity_form != 0 asks for the _dyn entry (edges_hint as
 * pgnn_dyn_count.hint, 0 = none) and returns PGNN_E_UNSUPPORTED where that
 * entry would.  Too small: PGNN_E_WORKSPACE, nothing launched.                */
#define PGNN_AGG_MAX 0
#define PGNN_AGG_SUM 1
#define PGNN_AGG_MEAN 2
/* gnn.py:362-365 with any of the three aggregators */
int pgnn_edge_mlp_scatter_agg_workspace_bytes(
    const pgnn_fc_layer *layers_host, int32_t n_layers, int32_t width,
    int64_t edges_cap, int64_t edges_hint, int32_t vertices_cap,
    int32_t aggregation, int32_t capacity_form, void *stream, size_t *bytes);
int pgnn_edge_mlp_scatter_agg_fwd(
    const float *P, const float *Q, int64_t ld_pq, int32_t width,
    const int32_t *edges, int64_t n_edges, int32_t num_vertices,
    const pgnn_fc_layer *layers_host, int32_t n_layers, int32_t edges_sorted,
    float *out, int64_t ld_out, int32_t *sched_ws, int32_t aggregation,
    void *workspace, size_t workspace_bytes, void *stream);
/* ... in capacity form; the finishing pass of the mean covers
 * min(*num_vertices, vertices_cap) rows */
int pgnn_edge_mlp_scatter_agg_fwd_dyn(
    const float *P, const float *Q, int64_t ld_pq, int32_t width,
    const int32_t *edges, int64_t edges_cap, int32_t vertices_cap,
    const pgnn_fc_layer *layers_host, int32_t n_layers, int32_t edges_sorted,
    float *out, int64_t ld_out, int32_t *sched_ws,
    const pgnn_dyn_count *n_edges, const pgnn_dyn_count *num_vertices,
    int32_t aggregation, void *workspace, size_t workspace_bytes, void *stream);
/* gnn.py:275-277 with any of the three aggregators (n_feat <= 13) */
int pgnn_point_set_pooling_agg_workspace_bytes(
    const pgnn_fc_layer *layers_host, int32_t n_layers, int32_t n_feat,
    int64_t edges_cap, int64_t edges_hint, int32_t keypoints_cap,
    int32_t aggregation, int32_t capacity_form, void *stream, size_t *bytes);
int pgnn_point_set_pooling_agg_fwd(
    const float *point_features, int32_t n_feat, const float *point_xyz,
    const int32_t *keypoint_indices, const int32_t *edges, int64_t n_edges,
    int32_t num_keypoints, const pgnn_fc_layer *layers_host, int32_t n_layers,
    int32_t edges_sorted, float *out, int64_t ld_out, int32_t *sched_ws,
    int32_t aggregation, void *workspace, size_t workspace_bytes, void *stream);
int pgnn_point_set_pooling_agg_fwd_dyn(
    const float *point_features, int32_t n_feat, const float *point_xyz,
    const int32_t *keypoint_indices, const int32_t *edges, int64_t edges_cap,
    int32_t keypoints_cap, const pgnn_fc_layer *layers_host, int32_t n_layers,
    int32_t edges_sorted, float *out, int64_t ld_out, int32_t *sched_ws,
    const pgnn_dyn_count *n_edges, const pgnn_dyn_count *num_keypoints,
    int32_t aggregation, void *workspace, size_t workspace_bytes, void *stream);

/* SECONDARY arithmetic for the same stage with ONE remaining edge layer of
 * 300x300 or 256x256 (csrc/edge_ws_split.h, Bf16x3): the layer's product runs on the
 * bf16 matrix pipe with BOTH operands split exactly into three bf16 parts
 * (8 + 8 + 8 significand bits) and the six products of combined order <= 2
 * accumulated in fp32 -- the dropped terms are below 2^-24 of a product, one
 * fp32 rounding (the weights' parts are rounded to nearest, the gathered
 * operand's first part too, its residual is cut in two); results agree with
 * the fp32-MFMA entry to fp32 rounding noise (not bit for bit) and are no
 * further from a float64 evaluation or from the reference's TF graphs
 * (tests/test_gpu_bf16x3.py, the edge_arith-parametrised parity tests).  The
 * fp32 entry above stays the
 * default and the parity reference (gnn.py:355-365 is fp32 in the reference).
 * `image`: device copy of what pgnn_pack_fc_bf16x3 wrote for the layer
 * (pgnn_packed_fc_bf16x3_bytes of it); width = the layer's k_in, n_out its
 * width, relu_from as in pgnn_fc_layer.  n_edges / num_vertices: NULL = the
 * capacities are the counts; else the capacity form (counts on the device).
 * PGNN_E_UNSUPPORTED, having done nothing, for other shapes, fewer than
 * ~65k edges (tunable b16_force lifts that) or P / Q of 4 GiB and more (rows
 * are addressed with 32-bit byte offsets): run pgnn_edge_mlp_scatter_max_fwd. */
size_t pgnn_packed_fc_bf16x3_bytes(int32_t k_in, int32_t n_out);
int pgnn_pack_fc_bf16x3(const float *w_host, const float *b_host, int32_t k_in,
                        int32_t n_out, void *image_host);
int pgnn_edge_mlp_scatter_max_bf16x3_fwd(
    const float *P, const float *Q, int64_t ld_pq, int32_t width,
    const int32_t *edges, int64_t edges_cap, int32_t vertices_cap,
    const void *image, int32_t n_out, int32_t relu_from, int32_t edges_sorted,
    float *out, int64_t ld_out, const pgnn_dyn_count *n_edges,
    const pgnn_dyn_count *num_vertices, void *stream);

/* SECONDARY arithmetic 'f16x2' for the same stage and shapes
 * (csrc/edge_ws_split.h, F16x2): both operands of the layer's product are represented
 * by TWO fp16 values (x ~ x0 + x1' / 2^11, round to nearest, 22 significand
 * bits), three fp16 MFMAs per block accumulate in fp32 -- half the matrix
 * instructions of the bf16x3 entry, three column groups instead of four.  Not
 * exact: each operand is within 2^-22 of its fp32 value (fp32's own rounding
 * is 2^-24); the stage's distance to a float64 evaluation grows by a few per
 * cent over the fp32 entry's (tests: the edge_arith-parametrised parity tests,
 * same bars as bf16x3).  Range: the gathered operand is clamped at 65504, and
 * bit 0 of *status (device int32, nullable; the caller zeroes it) is raised
 * when one COULD have reached 32768 (an element of the first num_vertices
 * rows of P or Q at or above 16384 in magnitude, or not a number: checked in
 * the kernel's prologue) -- rerun the stage through the fp32 entry then.
 * `image`: device copy of what pgnn_pack_fc_f16x2 wrote (it refuses weights
 * of magnitude >= 32768 with PGNN_E_UNSUPPORTED).  Otherwise as the bf16x3
 * entry, PGNN_E_UNSUPPORTED included.                                        */
size_t pgnn_packed_fc_f16x2_bytes(int32_t k_in, int32_t n_out);
int pgnn_pack_fc_f16x2(const float *w_host, const float *b_host, int32_t k_in,
                       int32_t n_out, void *image_host);
int pgnn_edge_mlp_scatter_max_f16x2_fwd(
    const float *P, const float *Q, int64_t ld_pq, int32_t width,
    const int32_t *edges, int64_t edges_cap, int32_t vertices_cap,
    const void *image, int32_t n_out, int32_t relu_from, int32_t edges_sorted,
    float *out, int64_t ld_out, int32_t *status, const pgnn_dyn_count *n_edges,
    const pgnn_dyn_count *num_vertices, void *stream);

/* The fp32 stage on SCALED operands (csrc/edge_ws.h, pk_sub_clamp): P, Q hold
 * 2^-scale_exp x the operands of pgnn_edge_mlp_scatter_max_fwd(_dyn) -- write
 * them with the per-vertex entries from weight images scaled by the same power
 * of two, which is exact.  The gather's packed subtraction then carries the
 * `clamp` modifier (to [0, 1]) and IS the ReLU: a third of the gather's VALU
 * instructions.  A power-of-two scale commutes with every rounding of the
 * chain, with ReLU and with max, and the kernel multiplies each closed
 * segment's maximum by 2^scale_exp before the bias add: `out` is, bit for
 * bit, what the plain entry writes for 2^scale_exp x P, 2^scale_exp x Q --
 * unless an intermediate of the plain chain is non-zero and below about
 * 2^(scale_exp - 102) in magnitude (the scaled value would be subnormal).
 * Guard: bit 0 of *status (device int32, nullable; the caller zeroes it) is
 * raised when an element of the first num_vertices rows of P or Q exceeds 0.5
 * in magnitude or is not a number (checked in the kernel's prologue; all
 * within 0.5 => no difference exceeds 1 and the clamp's upper bound never
 * acts).  The kernel still runs to the end then; `out` is finite but
 * unspecified: rerun the stage through the plain entry on unscaled operands.
 * scale_exp: 0..24.  n_edges / num_vertices: both NULL (the capacities are
 * the counts) or both given (capacity form).  layers / sched_ws / edges_sorted
 * as for the plain entry.  Returns PGNN_E_UNSUPPORTED, having done nothing,
 * where the weights-stationary kernel does not serve the launch -- exactly
 * where pgnn_edge_ws_applies says 0 for the expected edge count
 * (n_edges->hint, else edges_cap).
 *
 * PGNN_EDGE_K300_ORDER in `edges_sorted` (width = 300, a layer of 300 input
 * features): columns 288..303 of P and Q and rows 288..303 of the layer's image
 * come in the order of pgnn_k300_source -- position p holds feature
 * pgnn_k300_source(p); 291, 295, 299 and 303 are the zero padding -- as
 * pgnn_pack_fc_k300 writes the image; write P and Q from weight images whose
 * output columns are permuted the same way.  The padding is then the whole of
 * the last K group's fourth MFMA step, which the kernel does not issue: 7 of
 * every 532 MFMAs.  The real products keep their order in the fmaf chain and a
 * dropped one is fma(0, 0, acc), so `out` is what the entry writes without the
 * flag for the operands in natural order, bit for bit.  With the flag and any
 * other width or layer the entry returns PGNN_E_UNSUPPORTED, having done
 * nothing.  pgnn_pack_fc_k300 returns it for k_in != 300.
 *
 * pgnn_edge_ws_applies: *applies = 1 when a launch of the fp32 edge stage with
 * these layers, about `edges_expected` edges, on `stream` (its CU mask counts)
 * takes the weights-stationary kernel -- one 300x300 or 256x256 layer, ~65k
 * edges and more, a CU count the partition serves --, else 0.  Host only.    */
int pgnn_edge_ws_applies(const pgnn_fc_layer *layers_host, int32_t n_layers,
                         int32_t width, int64_t edges_expected, void *stream,
                         int32_t *applies);
#define PGNN_EDGE_K300_ORDER 4
int32_t pgnn_k300_source(int32_t position);
int pgnn_pack_fc_k300(const float *w_host, const float *b_host, int32_t k_in,
                      int32_t n_out, float *packed_host);
int pgnn_edge_mlp_scatter_max_scaled_fwd(
    const float *P, const float *Q, int64_t ld_pq, int32_t width,
    const int32_t *edges, int64_t edges_cap, int32_t vertices_cap,
    const pgnn_fc_layer *layers_host, int32_t n_layers, int32_t edges_sorted,
    float *out, int64_t ld_out, int32_t *sched_ws, int32_t scale_exp,
    int32_t *status, const pgnn_dyn_count *n_edges,
    const pgnn_dyn_count *num_vertices, void *stream);
/* Diagnostic: out[2i], out[2i+1] = the clamped packed subtraction above applied
 * to (a[2i], a[2i+1]) - (b[2i], b[2i+1]) for i < n_pairs <= 64, one wave
 * (device pointers): what the hardware makes of the modifier.               */
int pgnn_debug_pk_sub_clamp(const float *a, const float *b, float *out,
                            int32_t n_pairs, void *stream);

/* PointSetPooling (gnn.py:256-277) in the same SECONDARY arithmetic, for the
 * car point MLP 4 -> 32 -> 64 -> 128 -> 300 (csrc/pool_ws_f16.h): the three
 * narrow layers stay fp32 MFMA, the last layer's [E, 128] x [128, 300] product
 * -- 79 % of the stage's matrix time -- runs as three fp16 products per block
 * with both operands in two fp16 parts.  `layers` as for
 * pgnn_point_set_pooling_fwd (the last one's fp32 image is not read);
 * `last_image`: device copy of what pgnn_pack_fc_f16x2_acc wrote for the last
 * layer (the rows of W in the order a lane of the previous layer's fp32
 * accumulators holds them; same size as pgnn_packed_fc_f16x2_bytes);
 * `hidden_image` (nullable): the same for the 64 -> 128 layer below it, which
 * then runs in this arithmetic too (76 % of the remaining matrix time).  Counts
 * nullable (host-sized call) or both given (capacity form).  `status` as for
 * the edge entry.  Returns PGNN_E_UNSUPPORTED -- having done nothing -- for
 * other layer shapes or too few edges (tunable `b16_force` lifts the size
 * test): the caller takes pgnn_point_set_pooling_fwd(_dyn) then.            */
int pgnn_pack_fc_f16x2_acc(const float *w_host, const float *b_host,
                           int32_t k_in, int32_t n_out, void *image_host);
int pgnn_point_set_pooling_f16x2_fwd(
    const float *point_features, int32_t n_feat, const float *point_xyz,
    const int32_t *keypoint_indices, const int32_t *edges, int64_t edges_cap,
    int32_t keypoints_cap, const pgnn_fc_layer *layers, int32_t n_layers,
    const void *last_image, const void *hidden_image, int32_t edges_sorted,
    float *out, int64_t ld_out, int32_t *sched_ws, int32_t *status,
    const pgnn_dyn_count *n_edges, const pgnn_dyn_count *num_keypoints,
    void *stream);

/* Training forward of the same stage with ONE remaining edge layer: the fused
 * kernel also writes that layer's per-edge output rows [n_edges, ld_rows]
 * (the backward compares them with `out` to find the arg-max rows; rows and
 * maxima come from the same accumulators, so the winner reproduces `out` bit
 * for bit).  h1_out (nullable): the gathered hidden rows ReLU(P[src] -
 * Q[dst]) [n_edges, ld_pq] are written as well (= pgnn_edge_hidden_fwd).
 * Returns PGNN_E_UNSUPPORTED -- having done nothing -- when the
 * weights-stationary kernel does not apply (fewer than ~65k edges, layer
 * shapes other than 300x300 / 256x256): the caller then runs
 * pgnn_edge_hidden_fwd + pgnn_mlp_fwd + pgnn_scatter_max_f32.               */
int pgnn_edge_mlp_scatter_max_rows_fwd(const float *P, const float *Q,
                                       int64_t ld_pq, int32_t width,
                                       const int32_t *edges, int64_t n_edges,
                                       int32_t num_vertices,
                                       const pgnn_fc_layer *layer_host,
                                       int32_t edges_sorted, float *out,
                                       int64_t ld_out, float *rows_out,
                                       int64_t ld_rows, float *h1_out,
                                       void *stream);

/* x' = x + delta (gnn.py:346) and Q = x' @ Wx where Wx = the last 3 rows of
 * the first edge layer's weights (the rows that multiply the coordinate part
 * of the concat, gnn.py:350-352).  wx: device [3, ld_q] (zero padded).      */
int pgnn_offset_apply(const float *xyz, const float *delta, int64_t ld_delta,
                      int64_t n_rows, const float *wx, float *xyz_out,
                      float *Q, int64_t ld_q, void *stream);

/* Everything gnn.py:341-356 does per VERTEX before the per-edge work, in one
 * launch: delta = offset MLP(h[:, :c]) (n_offset_layers = 0: no auto offset,
 * delta = 0), Q = (xyz + delta) @ wx, P = [h[:, :c], xyz] @ W1 + b1
 * (p_layer: k_in = c + 3), and -- when agg is non-null -- the lowest() fill
 * of the [n_vertices, ld_agg] buffer the edge stage maxes into.  Equivalent
 * to pgnn_mlp_fwd (offset chain) + pgnn_offset_apply + pgnn_mlp_fwd (P) + fill
 * with identical arithmetic.  P, Q: [n_vertices, ld_pq], ld_pq = padded width
 * of p_layer's output; wx: device [3, ld_pq].                               */
int pgnn_vertex_pre_edge_fwd(const float *h, int64_t ld_h, int32_t c,
                             const float *xyz,
                             const pgnn_fc_layer *offset_layers_host,
                             int32_t n_offset_layers,
                             const pgnn_fc_layer *p_layer_host, const float *wx,
                             int64_t n_vertices, float *P, float *Q,
                             int64_t ld_pq, float *agg, int64_t ld_agg,
                             void *stream);
int pgnn_vertex_pre_edge_fwd_dyn(const float *h, int64_t ld_h, int32_t c,
                                 const float *xyz,
                                 const pgnn_fc_layer *offset_layers_host,
                                 int32_t n_offset_layers,
                                 const pgnn_fc_layer *p_layer_host,
                                 const float *wx, int64_t vertices_cap,
                                 float *P, float *Q, int64_t ld_pq, float *agg,
                                 int64_t ld_agg,
                                 const pgnn_dyn_count *n_vertices,
                                 void *stream);

/* Two per-vertex stages in ONE launch (small K: one 8-wave workgroup per
 * 16-row tile; PGNN_E_UNSUPPORTED -- having done nothing -- above ~32 rows per
 * CU or for chains wider than 320, the caller then runs the separate entries).
 * The reference evaluates them as separate TF ops on either side of an
 * operator boundary: the END of one layer -- PointSetPooling's output MLP
 * (gnn.py:279-283) or GraphNetAutoCenter's update MLP + residual
 * (gnn.py:367-372) -- and the START of the next GraphNetAutoCenter
 * (gnn.py:341-356: offset MLP, Q, P; see pgnn_vertex_pre_edge_fwd).
 *   y = front chain(x[:, :nx]) (+ residual)      -> [n_vertices, ld_y], always
 *                                                   written: it is the first
 *                                                   operator's output
 *   then pgnn_vertex_pre_edge_fwd on h = y.
 * Identical arithmetic to pgnn_mlp_fwd followed by pgnn_vertex_pre_edge_fwd
 * (the same MFMA sequence per output element): bit-identical results.
 * `agg` (the NEXT edge stage's aggregation buffer) must not alias `x`.       */
int pgnn_vertex_update_pre_edge_fwd(
    const float *x, int64_t ld_x, int32_t nx,
    const pgnn_fc_layer *front_layers_host, int32_t n_front,
    const float *residual, int64_t ld_res, float *y, int64_t ld_y, int32_t c,
    const float *xyz, const pgnn_fc_layer *offset_layers_host,
    int32_t n_offset_layers, const pgnn_fc_layer *p_layer_host, const float *wx,
    int64_t n_vertices, float *P, float *Q, int64_t ld_pq, float *agg,
    int64_t ld_agg, void *stream);
int pgnn_vertex_update_pre_edge_fwd_dyn(
    const float *x, int64_t ld_x, int32_t nx,
    const pgnn_fc_layer *front_layers_host, int32_t n_front,
    const float *residual, int64_t ld_res, float *y, int64_t ld_y, int32_t c,
    const float *xyz, const pgnn_fc_layer *offset_layers_host,
    int32_t n_offset_layers, const pgnn_fc_layer *p_layer_host, const float *wx,
    int64_t vertices_cap, float *P, float *Q, int64_t ld_pq, float *agg,
    int64_t ld_agg, const pgnn_dyn_count *n_vertices, void *stream);

/* The same for the model's last operator boundary: GraphNetAutoCenter's update
 * MLP + residual (gnn.py:367-372) followed by a second chain on its output --
 * the fused ClassAwarePredictor heads (gnn.py:133-163):
 *   y = front chain(x[:, :nx]) (+ residual)   -> [n_rows, ld_y], always written
 *   out = back chain(y[:, :ny])               -> [n_rows, ld_out]
 * = pgnn_mlp_fwd twice, bit-identical.  Same size limits as above.            */
int pgnn_mlp2_fwd(const float *x, int64_t ld_x, int32_t nx,
                  const pgnn_fc_layer *front_layers_host, int32_t n_front,
                  const float *residual, int64_t ld_res, float *y, int64_t ld_y,
                  int32_t ny, const pgnn_fc_layer *back_layers_host,
                  int32_t n_back, float *out, int64_t ld_out, int64_t n_rows,
                  void *stream);
int pgnn_mlp2_fwd_dyn(const float *x, int64_t ld_x, int32_t nx,
                      const pgnn_fc_layer *front_layers_host, int32_t n_front,
                      const float *residual, int64_t ld_res, float *y,
                      int64_t ld_y, int32_t ny,
                      const pgnn_fc_layer *back_layers_host, int32_t n_back,
                      float *out, int64_t ld_out, int64_t rows_cap,
                      const pgnn_dyn_count *rows, void *stream);

/* ---- training step (config 4: models.py:170-311, train.py:135-171,264-297,
 * 375-405, util/tf_util.py:3-43) ------------------------------------------
 * The backward pass needs the per-edge activations, so the training forward
 * materialises them with the primitives below (plus pgnn_mlp_fwd one layer at
 * a time and pgnn_scatter_max_f32); each primitive has an explicit adjoint.  */

/* Device-side pgnn_pack_fc (weights change every step).  transpose != 0 packs
 * W^T (the layer dX = dZ @ W^T of the backward pass; no bias).              */
int pgnn_pack_fc_device(const float *w, const float *b, int32_t k_in,
                        int32_t n_out, int32_t transpose, float *packed,
                        void *stream);

/* Every layer's device images refreshed in ONE launch (after pgnn_sgd_step):
 * `jobs_device` is a device array of n_jobs records
 *   struct { const float *w; const float *b; float *dst; int32_t k_in, n_out,
 *            kind, first_block, ld, reserved; }           (48 bytes each)
 * kind 0 = pgnn_pack_fc image of (w [k_in,n_out], b), 1 = image of w^T (no
 * bias), 2 = plain w^T as [n_out][16*ceil(k_in/16)] rows (zero padded; what
 * pgnn_segmax_fc_bwd_f32 reads), 3 = plain w as [k_in][16*ceil(n_out/16)]
 * rows (zero padded); 4 / 5 / 6 = strided block copy / block add / identity
 * (how the native trainer assembles its fused prediction-head matrices from
 * parameter blocks and hands their gradients back; `ld` = row stride of the
 * strided side).  A job covers ceil(elements / 256) blocks
 * of the launch; first_block is the running sum, total_blocks the grand
 * total.  The table is built once: the flat parameter buffer never moves.  */
int pgnn_pack_fc_many(const void *jobs_device, int32_t n_jobs,
                      int32_t total_blocks, void *stream);

/* H1[e] = ReLU(P[src(e)] - Q[dst(e)]) materialised, [n_edges, ld_pq].       */
int pgnn_edge_hidden_fwd(const float *P, const float *Q, int64_t ld_pq,
                         const int32_t *edges, int64_t n_edges, float *H1,
                         void *stream);
/* Adjoint: dP[src] += dH1, dQ[dst] -= dH1 (dH1 already masked by H1 > 0).
 * dP, dQ [n_vertices, ld] are zeroed by the call.                            */
int pgnn_edge_hidden_bwd(const float *dH1, int64_t ld, const int32_t *edges,
                         int64_t n_edges, int64_t n_vertices, float *dP,
                         float *dQ, void *stream);
/* batch_data (train.py:135-171): the frames of a batch merged into one
 * disjoint graph -- every array the concatenation of the frames' arrays,
 * keypoint indices and edge rows moved up by the points / centres of the
 * frames before them (`:150-160`) -- as ONE launch: job j copies n_words 4-byte
 * words from src to dst (device pointers; dst points INTO the merged array),
 * adding add0 to even and add1 to odd words as int32 (keypoint indices [k,1]:
 * add0 = add1 = points before; edge rows [E,2]: add0 = points before, add1 =
 * centres before; float arrays: 0, 0).  jobs_host is a HOST array. */
typedef struct pgnn_merge_job {
  const void *src;
  void *dst;
  int64_t n_words;
  int32_t add0, add1;
} pgnn_merge_job;
int pgnn_merge_rows(const pgnn_merge_job *jobs_host, int32_t n_jobs,
                    void *stream);
/* Two capacity-form frames (graph_gen's deferred_counts) merged into one, on
 * the device: what batch_data does for host-sized frames, for frames whose
 * sizes exist only in their count records.  A record is int32 [2 + 2 L]: K,
 * kd-tree status, then (rows written, rows required) per edge level.
 *   - points [n_points, 3] / features [n_points, n_feat]: host-known rows; B's
 *     follow A's at row a->n_points;
 *   - kp_xyz [kp_cap, 3] / kp_idx [kp_cap]: the first K rows exist; B's rows
 *     follow A's at row K_A (read from A's record), indices + a->n_points;
 *   - edges[l] [edge_caps[l], 2] (source, centre), l < n_levels <=
 *     PGNN_MERGE_MAX_LEVELS: the first `rows written` exist; B's follow A's,
 *     centres + K_A, sources + a->n_points on level 0 (points -> keypoints)
 *     and + K_A above it (keypoints -> keypoints).  Lists grouped by ascending
 *     centre stay grouped;
 *   - merged->counts: the merged record in the same layout: sums of K, of the
 *     rows written (as far as the merged capacities hold them) and of the rows
 *     required, so a frame whose list overflowed its capacity shows in the
 *     merged record too; status: A's if non-zero, else B's.
 * Only the first `count` rows of an input are read, rows behind the merged
 * counts are not written, nothing is read back; one launch.  merged->n_points
 * must be a->n_points + b->n_points.  words_hint (0: none): the expected
 * length, in 4-byte words, of the longest list; it sizes the grid only.      */
#define PGNN_MERGE_MAX_LEVELS 4
typedef struct pgnn_frame_arrays {
  int32_t *counts;
  float *points;
  float *features;
  int64_t n_points;
  float *kp_xyz;
  int32_t *kp_idx;
  int64_t kp_cap;
  int32_t *edges[PGNN_MERGE_MAX_LEVELS];
  int64_t edge_caps[PGNN_MERGE_MAX_LEVELS];
} pgnn_frame_arrays;
int pgnn_merge_frames_dyn(const pgnn_frame_arrays *a_host,
                          const pgnn_frame_arrays *b_host,
                          const pgnn_frame_arrays *merged_host, int32_t n_feat,
                          int32_t n_levels, int64_t words_hint, void *stream);
/* PointSetPooling edge features [f(src), xyz(src) - xyz(kp(dst)), 0...] as a
 * [n_edges, 16] matrix (gnn.py:256-267).                                     */
int pgnn_pool_features_fwd(const float *point_features, int32_t n_feat,
                           const float *point_xyz,
                           const int32_t *keypoint_indices,
                           const int32_t *edges, int64_t n_edges, float *F,
                           void *stream);
/* The same rows for any feature width, [n_edges, ld_f >= n_feat + 3] with zero
 * pad columns, from features with row stride ld_features: a PointSetPooling
 * above the first pooling level gathers the previous level's (300-wide)
 * vertex features, which the fused pooling kernel (n_feat <= 13) does not
 * take -- pgnn_pool_features_wide_fwd + pgnn_mlp_fwd + pgnn_scatter_max_f32
 * are the operator then (no shipped config).                                 */
int pgnn_pool_features_wide_fwd(const float *point_features,
                                int64_t ld_features, int32_t n_feat,
                                const float *point_xyz,
                                const int32_t *keypoint_indices,
                                const int32_t *edges, int64_t n_edges, float *F,
                                int64_t ld_f, void *stream);
/* dY[i] = (Y[i] > 0) ? dY[i] : 0 in place (tf ReluGrad), over `count` floats. */
int pgnn_relu_mask_mul(float *dY, const float *Y, int64_t count, void *stream);
/* Gradient of tf.math.unsorted_segment_max (TF's
 * _UnsortedSegmentMinOrMaxGrad): rows equal to their segment's max share the
 * segment's gradient equally.  relu_mask != 0 additionally zeroes rows whose
 * value is not > 0 (fused ReluGrad of the layer that produced `data`).
 * tie_count_ws: int32 [num_segments * n_cols] scratch.                       */
int pgnn_scatter_max_bwd_f32(const float *data, int64_t ld_data,
                             const int32_t *seg_ids, int64_t n_rows,
                             int32_t n_cols, int32_t num_segments,
                             const float *out, int64_t ld_out,
                             const float *grad_out, int64_t ld_grad_out,
                             int32_t *tie_count_ws, float *grad_data,
                             int64_t ld_grad_data, int32_t relu_mask,
                             void *stream);
/* Adjoint of  out = unsorted_segment_max(Y),  Y = ReLU(X W + b)  -- the last
 * per-edge layer and the aggregation of PointSetPooling (gnn.py:269-277) and
 * GraphNetAutoCenter (gnn.py:357-365) -- exploiting that the max passes its
 * gradient to one row per (segment, column): ~num_segments*n_cols non-zeros
 * among n_rows*n_cols, so neither dZ nor the two n_rows-sized GEMMs of the
 * dense adjoint are formed.  Same result as pgnn_scatter_max_bwd_f32
 * (relu_mask = 1: TF's tie rule, ReluGrad) followed by dX = dZ W^T (masked by
 * X > 0 when mask_x != 0: the ReluGrad of the layer that produced X) and
 * dW += X^T dZ, db += column sums of dZ, up to float32 summation order.
 *   Y [n_rows, ld_y], out [num_segments, ld_out]: 16-byte aligned rows padded
 *   to a multiple of 4 columns; X [n_rows, ld_x] (k_in features);
 *   WT = W^T as [n_cols][ld_wt] (pgnn_pack_fc_many kind 2);
 *   dX [n_rows, ld_dx] (nullable): dx_cols columns written (zeros beyond k_in);
 *   dW [k_in, n_cols] and db [n_cols] (nullable) are ACCUMULATED into.       */
size_t pgnn_segmax_fc_bwd_workspace_bytes(int64_t n_rows, int32_t n_cols,
                                          int32_t num_segments, int32_t k_in);
int pgnn_segmax_fc_bwd_f32(const float *Y, int64_t ld_y,
                           const int32_t *seg_ids, int64_t n_rows,
                           int32_t n_cols, int32_t num_segments,
                           const float *out, int64_t ld_out,
                           const float *grad_out, int64_t ld_go,
                           const float *X, int64_t ld_x, int32_t k_in,
                           const float *WT, int64_t ld_wt, float *dX,
                           int64_t ld_dx, int32_t dx_cols, int32_t mask_x,
                           float *dW, float *db, void *workspace,
                           size_t workspace_bytes, void *stream);
/* The GraphNetAutoCenter form (gnn.py:348-365): X = H1 = ReLU(P[src] - Q[dst])
 * [n_edges, ld_h1] feeds the layer, so the routed gradient is scattered
 * straight into dP[src] += g, dQ[dst] -= g (both [num_vertices, ld_pq], zeroed
 * by the call: pgnn_edge_hidden_bwd's outputs) and dH1 is never written.
 * edges [n_edges, 2] = (src, dst) grouped by dst for the in-register dQ runs
 * (any order is correct); dst_ids = its dst column, contiguous.  H1 may be
 * NULL (the fused training forward pgnn_edge_mlp_scatter_max_rows_fwd never
 * writes it): its rows are then recomputed from P and Q [num_vertices,
 * ld_pq] as ReLU(P[src] - Q[dst]).                                          */
int pgnn_edge_segmax_fc_bwd_f32(const float *Y, int64_t ld_y,
                                const int32_t *edges, const int32_t *dst_ids,
                                int64_t n_edges, int32_t n_cols,
                                int32_t num_vertices, const float *out,
                                int64_t ld_out, const float *grad_out,
                                int64_t ld_go, const float *H1, int64_t ld_h1,
                                const float *P, const float *Q, int32_t k_in,
                                const float *WT, int64_t ld_wt,
                                float *dP, float *dQ, int64_t ld_pq, float *dW,
                                float *db, void *workspace,
                                size_t workspace_bytes, void *stream);
/* dW [k_in, n_out] (= X^T dZ) and db [n_out] (= column sums of dZ; may be
 * NULL) of y = x W + b, deterministic (fixed-order slice reduction).
 * accumulate != 0 adds to dW/db.                                             */
size_t pgnn_weight_grad_workspace_bytes(int32_t k_in, int32_t n_out,
                                        int64_t n_rows);
int pgnn_weight_grad_f32(const float *X, int64_t ld_x, int32_t k_in,
                         const float *dZ, int64_t ld_dz, int32_t n_out,
                         int64_t n_rows, float *dW, float *db,
                         int32_t accumulate, void *workspace,
                         size_t workspace_bytes, void *stream);
/* Fused backward of PointSetPooling's narrow point-MLP layers for the shipped
 * car chain feat -> 32 -> 64 -> 128 (gnn.py:256-277 under tf.gradients): given
 * the gradient w.r.t. the third layer's pre-activation (what
 * pgnn_segmax_fc_bwd_f32 hands over for the 128 -> 300 layer), the weight and
 * bias gradients of all three layers in one pass over the E rows -- the two dX
 * products and ReLU masks in between happen in LDS.  feat [E,16] (k_in0 <= 15
 * columns used), act0 [E,32], act1 [E,64], dz2 [E,128]: contiguous rows;
 * w2t_packed / w1t_packed: the TRANSPOSED images (pgnn_pack_fc_many kind 1) of
 * the 64 -> 128 and 32 -> 64 layers.  Deterministic (fixed slice order).     */
size_t pgnn_pool_narrow_bwd_workspace_bytes(int64_t n_rows);
int pgnn_pool_narrow_bwd_f32(const float *feat, const float *act0,
                             const float *act1, const float *dz2,
                             int64_t n_rows, const float *w2t_packed,
                             const float *w1t_packed, int32_t k_in0, float *dW0,
                             float *db0, float *dW1, float *db1, float *dW2,
                             float *db2, int32_t accumulate, void *workspace,
                             size_t workspace_bytes, void *stream);
/* The same for MANY small layers in one launch pair (train.py:264-297 asks
 * tf.gradients for every variable at once; here the K-row layers of a step --
 * ~25 GEMMs of [k_in x K] x [K x n_out], K ~ 2 000 vertices -- would each be a
 * latency-bound launch plus a reduce: 0.7 ms of a 4.7 ms step).  jobs: a HOST
 * array; 1 <= n_out <= 320 per job; dW is [k_in, n_out] contiguous; the
 * outputs of different jobs must not overlap (they are written by one launch).  Fixed
 * slice partition and reduction order: deterministic, not bit-equal to
 * pgnn_weight_grad_f32 (other slice boundaries).                           */
typedef struct pgnn_wgrad_job {
  const float *X;   /* [n_rows, ld_x] layer input                           */
  int64_t ld_x;
  const float *dZ;  /* [n_rows, ld_dz] gradient w.r.t. the pre-activation    */
  int64_t ld_dz;
  int64_t n_rows;
  float *dW;        /* [k_in, n_out]                                         */
  float *db;        /* [n_out] or NULL                                       */
  int32_t k_in, n_out;
  int32_t accumulate, reserved;
} pgnn_wgrad_job;
size_t pgnn_weight_grad_many_workspace_bytes(const pgnn_wgrad_job *jobs_host,
                                             int32_t n_jobs);
int pgnn_weight_grad_many_f32(const pgnn_wgrad_job *jobs_host, int32_t n_jobs,
                              void *workspace, size_t workspace_bytes,
                              void *stream);
/* models.py:212-255 (cls 'softmax', loc 'huber_loss', delta 1):
 * sums4 (device, 4 doubles) = {sum_v CE_v, sum_v mean_7 huber_v*valid_v,
 * n_vertices, sum valid}; dlogits [n, nc] / dpred_box [n, nc, box_len]
 * receive the gradients of cls_grad_scale*sum CE + loc_grad_scale*sum loc
 * (the caller folds loss weights and the global 1/N, 1/N_valid of
 * train.py:264-288 into the two scales).                                     */
int pgnn_loss_fwd_bwd(const float *logits, int64_t ld_logits,
                      const int32_t *labels, const float *pred_box,
                      int32_t box_len, const float *gt_box, const float *valid,
                      int64_t n_vertices, int32_t num_classes,
                      float cls_grad_scale, float loc_grad_scale,
                      double *sums4, float *dlogits, float *dpred_box,
                      void *stream);
/* The same with the GLOBAL endpoint counts of train.py:268-284 on the device
 * (counts2 = {num_endpoint, num_valid_endpoint} as doubles, e.g. fresh out of
 * an all-reduce over the ranks): the kernel forms cls_loss_weight /
 * num_endpoint and loc_loss_weight / num_valid_endpoint itself (0 for a zero
 * count: tf.math.div_no_nan), so no host read sits between the forward and the
 * backward pass of a multi-rank step.                                         */
int pgnn_loss_fwd_bwd_counts(const float *logits, int64_t ld_logits,
                             const int32_t *labels, const float *pred_box,
                             int32_t box_len, const float *gt_box,
                             const float *valid, int64_t n_vertices,
                             int32_t num_classes, double cls_loss_weight,
                             double loc_loss_weight, const double *counts2,
                             double *sums4, float *dlogits, float *dpred_box,
                             void *stream);
/* The same pass with the other per-vertex classification losses of
 * models.py:210-228 and the per-class localisation weights of :240-246:
 * cls_kind 0 'softmax' (as above), 1 'focal_softmax' (models/loss.py:31-48:
 * (1 - p_label)^gamma * CE), 2 'focal_sigmoid' (models/loss.py:5-29: per-class
 * sigmoid CE * (1 - p_t)^gamma * (alpha | 1 - alpha), averaged over the classes
 * as well, models.py:229).  class_loc_weight (nullable, device float
 * [num_classes]): 'classwise_loc_loss_weight' of loc_loss_kwargs, applied to a
 * vertex's Huber terms by its label.  counts2 nullable: null = the host-scale
 * form (cls_grad_scale / loc_grad_scale used), else the _counts form.
 * gamma == 0 is plain CE / sigmoid CE (TF's pow(0, 0) = 1); for 0 < gamma < 1
 * the derivative's (1 - p_t)^(gamma - 1) is evaluated at max(1 - p_t, 1e-6).
 * 'top_k_softmax' / 'top_k_huber_loss': pgnn_loss_fwd_bwd_sel below.         */
int pgnn_loss_fwd_bwd_ex(const float *logits, int64_t ld_logits,
                         const int32_t *labels, const float *pred_box,
                         int32_t box_len, const float *gt_box,
                         const float *valid, int64_t n_vertices,
                         int32_t num_classes, float cls_grad_scale,
                         float loc_grad_scale, const double *counts2,
                         double cls_loss_weight, double loc_loss_weight,
                         int32_t cls_kind, float alpha, float gamma,
                         const float *class_loc_weight, double *sums4,
                         float *dlogits, float *dpred_box, void *stream);
/* The top-k variants (models.py:222-228 'top_k_softmax', :266-291
 * 'top_k_huber_loss') in three steps, all on the device:
 *   1. pgnn_loss_fwd_bwd_sel with point_cls / point_loc set (no gradients):
 *      the per-vertex classification loss and the per-vertex mean Huber loss
 *      (valid and class weights applied) -- what the reference hands to
 *      tf.math.top_k;
 *   2. pgnn_topk_mask_f32: mask[i] = 1 for the k largest values (equal values:
 *      lower index first, like tf.math.top_k), 0 elsewhere; k > n is an error
 *      as in TF;
 *   3. pgnn_loss_fwd_bwd_sel with select_cls / select_loc = those masks: a
 *      vertex outside a selection adds no loss and gets no gradient;
 *      sums4[3] counts the valid vertices INSIDE the loc selection
 *      (models.py:283-285); cls_sum_weight scales the classification sum and
 *      its gradient -- n / k turns the mean over n the callers divide by into
 *      the reference's mean over the k selected values (with towers /
 *      unify_copies, train.py:268-284: n_rank / k on every rank).
 * Every pointer after class_loc_weight is nullable; with all of them null and
 * cls_sum_weight 1 this is pgnn_loss_fwd_bwd_ex. */
int pgnn_loss_fwd_bwd_sel(const float *logits, int64_t ld_logits,
                          const int32_t *labels, const float *pred_box,
                          int32_t box_len, const float *gt_box,
                          const float *valid, int64_t n_vertices,
                          int32_t num_classes, float cls_grad_scale,
                          float loc_grad_scale, const double *counts2,
                          double cls_loss_weight, double loc_loss_weight,
                          int32_t cls_kind, float alpha, float gamma,
                          const float *class_loc_weight,
                          const float *select_cls, const float *select_loc,
                          float cls_sum_weight, float *point_cls,
                          float *point_loc, double *sums4, float *dlogits,
                          float *dpred_box, void *stream);
size_t pgnn_topk_mask_workspace_bytes(int64_t n);
int pgnn_topk_mask_f32(const float *values, int64_t n, int64_t k, float *mask,
                       void *workspace, size_t workspace_bytes, void *stream);
/* params -= lr * (grad_scale*grads + l1_scale*sign(params)*is_weight)
 * (GradientDescentOptimizer + slim.l1_regularizer on FC weights only).       */
int pgnn_sgd_step(float *params, const float *grads, const float *is_weight,
                  int64_t n, float lr, float grad_scale, float l1_scale,
                  void *stream);
/* The other optimizers train.py:380-391 offers, TF 1.x update rules on the same
 * flat buffers (gradient = grad_scale*grads + l1_scale*sign(params)*is_weight
 * as above; slot0 / slot1: optimizer state with the parameters' layout):
 *   kind 1 MomentumOptimizer (h0 = momentum, no Nesterov): slot0 = accumulator
 *   kind 2 RMSPropOptimizer (h0 = momentum, h1 = decay, h2 = epsilon; not
 *          centered): slot0 = ms (TF initialises it to ONES), slot1 = mom
 *   kind 3 AdamOptimizer (h0 = beta1, h1 = beta2, h2 = epsilon): slot0 = m,
 *          slot1 = v; `lr` is the caller's bias-corrected
 *          lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = 1, 2, ...            */
int pgnn_optimizer_step(int32_t kind, float *params, const float *grads,
                        const float *is_weight, float *slot0, float *slot1,
                        int64_t n, float lr, float grad_scale, float l1_scale,
                        float h0, float h1, float h2, void *stream);
/* *out (device double) = sum |params| over is_weight entries (reg_loss/scale). */
int pgnn_l1_norm(const float *params, const float *is_weight, int64_t n,
                 double *out, void *stream);
/* The other weight regularizers of models.py:11-15 (tf.contrib.layers):
 * l2_regularizer(scale) = scale * sum(w^2) / 2 (tf.nn.l2_loss),
 * l1_l2_regularizer(scale_l1, scale_l2) = the sum of the two; FC weights only
 * (models.py:114-115).  The two entries above with the gradient
 *   grad_scale*grads + (l1_scale*sign(params) + l2_scale*params)*is_weight;
 * l2_scale = 0 is exactly pgnn_sgd_step / pgnn_optimizer_step (they forward
 * here).                                                                      */
int pgnn_sgd_step_l1l2(float *params, const float *grads, const float *is_weight,
                       int64_t n, float lr, float grad_scale, float l1_scale,
                       float l2_scale, void *stream);
int pgnn_optimizer_step_l1l2(int32_t kind, float *params, const float *grads,
                             const float *is_weight, float *slot0, float *slot1,
                             int64_t n, float lr, float grad_scale,
                             float l1_scale, float l2_scale, float h0, float h1,
                             float h2, void *stream);
/* out2 (device double[2]) = {sum |params|, sum params^2} over is_weight entries:
 * reg_loss = l1_scale * out2[0] + l2_scale * out2[1] / 2.                     */
int pgnn_weight_norms(const float *params, const float *is_weight, int64_t n,
                      double *out2, void *stream);

/* ---- native training step (config 4) ----------------------------------------
 * What train.py builds with TF towers -- model.predict with saved
 * activations, tf.gradients of model.loss (models.py:79-163, 170-311;
 * train.py:225-297) -- as ONE object on the device: the whole forward and the
 * whole backward are two calls, every kernel launch inside is issued from C++.
 * (The Python mirror keeps a step composed of the primitives above; tests hold
 * the two to the same gradients.)
 *
 * The model is described by where each fully connected layer lives in the
 * caller's FLAT parameter buffer (reference variable order, [k_in, n_out]
 * row-major weights, then biases): offsets in floats.  Gradients go to a flat
 * buffer of the same layout and are ACCUMULATED (zero it per step).          */
#define PGNN_TRAIN_MAX_FC 8
#define PGNN_TRAIN_MAX_STAGES 8
#define PGNN_TRAIN_MAX_CLASSES 16
#define PGNN_TRAIN_MAX_LEVELS 4
typedef struct pgnn_train_fc {
  int64_t w_off, b_off; /* float offsets of weights / biases in the flat buffer */
  int32_t k_in, n_out;
} pgnn_train_fc;
typedef struct pgnn_train_stage {
  int32_t kind;        /* 0 = scatter_max_point_set_pooling (gnn.py:222-283),
                          1 = scatter_max_graph_auto_center_net (gnn.py:298-373) */
  int32_t graph_level; /* index into the batch's coords / keypoints / edges     */
  int32_t n_a, n_b, n_c, reserved;
  pgnn_train_fc a[PGNN_TRAIN_MAX_FC]; /* point MLP / edge MLP (all ReLU)        */
  pgnn_train_fc b[PGNN_TRAIN_MAX_FC]; /* output MLP (ReLU) / update MLP (last
                                         layer linear, + residual)             */
  pgnn_train_fc c[PGNN_TRAIN_MAX_FC]; /* auto-offset MLP, last layer linear;
                                         n_c = 0: auto_offset False            */
} pgnn_train_stage;
typedef struct pgnn_train_model {
  int32_t n_stages, num_classes, box_len, reserved;
  int64_t n_params;
  pgnn_train_stage stages[PGNN_TRAIN_MAX_STAGES];
  pgnn_train_fc cls[2];                          /* C -> hw -> nc (gnn.py:145-152)  */
  pgnn_train_fc loc[PGNN_TRAIN_MAX_CLASSES][3];  /* per class C -> hw -> hw -> L   */
  /* which columns of the C-wide features box head j reads: 0 = all of them
   * (ClassAwarePredictor, gnn.py:133-163; what a zero-initialised model
   * means), 1 = its own slice [j*s, (j+1)*s), s = C / num_classes, so that
   * loc[j][0].k_in = s (ClassAwareSeparatedPredictor, gnn.py:178-213: tf.split).
   * The class head reads all C columns either way.                            */
  int32_t loc_split, reserved2;
} pgnn_train_model;
typedef struct pgnn_train_batch { /* device pointers; what train.py's batch_data
                                     returns for this rank (train.py:135-171) */
  const float *input_v;           /* [n_vertices[0], n_feat]                   */
  int32_t n_feat, n_levels;
  int64_t n_vertices[PGNN_TRAIN_MAX_LEVELS + 1];
  const float *coords[PGNN_TRAIN_MAX_LEVELS + 1];   /* [n_vertices[l], 3]      */
  const int32_t *keypoints[PGNN_TRAIN_MAX_LEVELS];  /* [n_vertices[l + 1]]     */
  const int32_t *edges[PGNN_TRAIN_MAX_LEVELS];      /* [n_edges[l], 2]         */
  int64_t n_edges[PGNN_TRAIN_MAX_LEVELS];
  int32_t edges_sorted[PGNN_TRAIN_MAX_LEVELS];      /* grouped by ascending dst */
} pgnn_train_batch;

int pgnn_trainer_create(const pgnn_train_model *model_host, void **handle);
int pgnn_trainer_destroy(void *handle);
/* Device images of the weights (MFMA fragment order forward / transposed,
 * plain W^T of the sparse-adjoint layers, fused prediction heads) + the job
 * table that refreshes them: the caller allocates images_bytes once and binds
 * the flat buffers (they must not move afterwards).  bind packs once;
 * repack after every parameter update (one launch). */
size_t pgnn_trainer_images_bytes(void *handle);
int pgnn_trainer_bind(void *handle, float *params, float *grads, void *images,
                      size_t images_bytes, void *stream);
int pgnn_trainer_repack(void *handle, void *stream);
/* Scratch of one forward + backward on a batch of these sizes (saved
 * activations included). */
size_t pgnn_trainer_workspace_bytes(void *handle, const pgnn_train_batch *batch);
/* Forward with saved activations.  *logits / *pred_box point INTO the
 * workspace (valid until the next forward on it): logits [K, *ld_logits]
 * (num_classes columns used), pred_box [K, num_classes, box_len] contiguous. */
int pgnn_trainer_forward(void *handle, const pgnn_train_batch *batch,
                         void *workspace, size_t workspace_bytes,
                         const float **logits, int64_t *ld_logits,
                         const float **pred_box, void *stream);
/* Backward of the forward last run on `workspace`: dlogits [K, num_classes]
 * and dpred_box [K, num_classes, box_len] (what pgnn_loss_fwd_bwd wrote) ->
 * gradients accumulated into the bound flat gradient buffer. */
int pgnn_trainer_backward(void *handle, const pgnn_train_batch *batch,
                          void *workspace, size_t workspace_bytes,
                          const float *dlogits, const float *dpred_box,
                          void *stream);

/* Backward + the step's collectives in one call: pgnn_trainer_backward, then
 * -- when `comm` is not null -- pgnn_allreduce_step(comm, <bound gradient
 * buffer>, n_params, sums, n_sums) on the same stream: nothing of the host
 * between the last gradient kernel and the all-reduce's launch.  comm null:
 * exactly pgnn_trainer_backward. */
int pgnn_trainer_backward_sync(void *handle, const pgnn_train_batch *batch,
                               void *workspace, size_t workspace_bytes,
                               const float *dlogits, const float *dpred_box,
                               void *comm, double *sums, int64_t n_sums,
                               void *stream);

/* ---- collectives (config 4) ---------------------------------
 * One process per GPU.  Replaces the reference's in-process towers:
 * `average_gradients` (util/tf_util.py:3-43: concat the towers' gradients on a
 * new axis, reduce_mean over it) behind `unify_copies` (train.py:264-288:
 * every tower's cls / loc loss re-weighted by the GLOBAL endpoint counts) and
 * the single apply_gradients (train.py:397-405).  With every rank's loss
 * already divided by the global counts, the towers' mean x world = the SUM of
 * the ranks' gradients: one all-reduce(sum) of the flat fp32 gradient buffer
 * (1 489 609 floats = 5.96 MB for car_auto_T3; latency-bound on xGMI, hence
 * one call and no bucketing), and one of the counts / loss sums (float64).
 *
 * The communicator is RCCL's, bound at run time (dlopen of the RCCL image the
 * process already holds, else the system's librccl.so.1; PGNN_RCCL_LIB names
 * another).  Rank 0 calls pgnn_comm_unique_id and hands the
 * PGNN_COMM_ID_BYTES bytes to the other ranks by whatever the launcher offers
 * (a file, a torch.distributed store, MPI); then EVERY rank calls
 * pgnn_comm_init_rank (collective, blocking; uses the calling thread's current
 * HIP device).  The collectives are in place, asynchronous, ordered on
 * `stream` like every other entry; a world of one rank is valid (and still
 * enters RCCL).  Errors: PGNN_E_COMM with RCCL's message in pgnn_last_error. */
#define PGNN_COMM_ID_BYTES 128
int pgnn_comm_unique_id(void *id_host);
int pgnn_comm_init_rank(const void *id_host, int32_t world, int32_t rank,
                        void **comm_out);
int pgnn_comm_destroy(void *comm);
/* world / rank of `comm` (nullable: version only) and RCCL's version code
 * (e.g. 22606); each output nullable. */
int pgnn_comm_info(void *comm, int32_t *world, int32_t *rank,
                   int32_t *rccl_version);
/* Which RCCL image is bound (path or "<soname> (already loaded)"), or why none. */
const char *pgnn_comm_library(void);
/* 0, or PGNN_E_COMM with the asynchronous error RCCL recorded for `comm`. */
int pgnn_comm_async_error(void *comm);
/* buf[i] = sum over ranks of buf[i], in place. */
int pgnn_allreduce_sum_f32(void *comm, float *buf, int64_t n, void *stream);
int pgnn_allreduce_sum_f64(void *comm, double *buf, int64_t n, void *stream);
/* The step's two reductions as ONE RCCL group (one launch): the flat gradient
 * (fp32) and the loss sums / endpoint counts (float64).  Either may be empty. */
int pgnn_allreduce_step(void *comm, float *grads, int64_t n_grads, double *sums,
                        int64_t n_sums, void *stream);
/* buf of `root` -> every rank (initial weights of a run that was not resumed
 * from one checkpoint: the reference's towers share ONE set of variables,
 * train.py:225-227 under `reuse`). */
int pgnn_broadcast_f32(void *comm, float *buf, int64_t n, int32_t root,
                       void *stream);

/* ---- detection post-processing (the step right after
 * the path; run.py:264-326).  All arrays are device pointers.
 *
 * Box codec `classaware_all_class_box_encoding` (box_encoding.py:231-299), the
 * method of every shipped config.  cls_labels [n_rows] int32; xyz [n_rows,3];
 * boxes / encoded [n_rows, boxes_per_row, 7] = (x,y,z,l,h,w,yaw).  class_table
 * [n_table,5] rows = {l, h, w, yaw_offset, active}: row `label` describes how a
 * row with that label is (de)normalised -- the host builds it from label_map
 * and median_object_size_map (label -> median size, yaw_offset 0; label+1 ->
 * same size, yaw_offset pi/2).  Like the reference only box column 0 is class
 * scaled; the xyz offset applies to every column. */
int pgnn_box_decode_f32(const int32_t *cls_labels, const float *xyz,
                        const float *encoded, const float *class_table,
                        int32_t n_table, int64_t n_rows, int32_t boxes_per_row,
                        float *decoded, void *stream);
int pgnn_box_encode_f32(const int32_t *cls_labels, const float *xyz,
                        const float *boxes, const float *class_table,
                        int32_t n_table, int64_t n_rows, int32_t boxes_per_row,
                        float *encoded, void *stream);
/* Box codec `classaware_all_class_box_canonical_encoding`: the same arguments,
 * class table and pass-through rules (columns >= 1 and inactive labels get the
 * xyz offset only), with the vertex->centre offset expressed in the anchor's
 * own frame.  a = the yaw relative to the anchor (yaw - yaw_offset when
 * encoding, e6*pi/4 when decoding); (p, q) = (l, w) for a horizontal anchor
 * and (w, l) for a vertical one, the reference's swap.  cos/sin/exp/log are
 * evaluated in double on the float32 argument and rounded once; products, sums
 * and quotients are float32 in the reference's order.
 * Replaces box_encoding.py:345-395 (classaware_all_class_box_canonical_decoding):
 *   out0 = e0*p*cos a + e2*q*sin a, out2 = -e0*p*sin a + e2*q*cos a, + xyz. */
int pgnn_box_decode_canonical_f32(const int32_t *cls_labels, const float *xyz,
                                  const float *encoded,
                                  const float *class_table, int32_t n_table,
                                  int64_t n_rows, int32_t boxes_per_row,
                                  float *decoded, void *stream);
/* Replaces box_encoding.py:301-343 (classaware_all_class_box_canonical_encoding):
 *   d = box - xyz, out0 = (d0*cos a - d2*sin a)/p, out2 = (d0*sin a + d2*cos a)/q,
 *   out6 = a/(pi/4). */
int pgnn_box_encode_canonical_f32(const int32_t *cls_labels, const float *xyz,
                                  const float *boxes, const float *class_table,
                                  int32_t n_table, int64_t n_rows,
                                  int32_t boxes_per_row, float *encoded,
                                  void *stream);
/* run.py:266-290: candidates of probs [n_vertices, num_classes] = flat indices
 * p = k*num_classes + c with 0 < c < num_classes-1 and prob > 1/num_classes,
 * ascending (np.nonzero order).  out_label holds the merged class of
 * run.py:287-289 (2->1, 4->3, 6->5).  *out_count (device) receives the full
 * count even when it exceeds `capacity` (entries beyond it are dropped). */
int pgnn_detection_candidates(const float *probs, int64_t n_vertices,
                              int32_t num_classes, int32_t *out_index,
                              int32_t *out_label, int64_t capacity,
                              int32_t *out_count, void *stream);
/* The same for a capacity-form frame (the frame loop keeps frames in flight
 * and reads nothing between the GNN and this call): probs has n_vertices_cap
 * rows of which the first *n_vertices_dev (a device int32, the K of the
 * frame's count record) exist. */
int pgnn_detection_candidates_dyn(const float *probs, int64_t n_vertices_cap,
                                  const int32_t *n_vertices_dev,
                                  int32_t num_classes, int32_t *out_index,
                                  int32_t *out_label, int64_t capacity,
                                  int32_t *out_count, void *stream);
/* nms.py:241-300.  mode: 0 = nms_boxes_3d (plain; integer corners scaled by
 * appr_factor, nms.py:113-115), 1 = nms_boxes_3d_uncertainty (median merge +
 * score accumulation, what run.py uses), 2 = nms_boxes_3d_merge_only,
 * 3 = nms_boxes_3d_score_only; the overlap is overlapped_boxes_3d_fast_poly
 * (nms.py:64-88).  Boxes are ordered by descending score (ties: input order),
 * cut to top_k when top_k > 0, then scanned like the reference loop.  Outputs
 * (capacity n_boxes each) are the kept boxes in score order; attributes
 * (nullable -> arange) ride along; *out_count (device) = number kept. */
size_t pgnn_nms_workspace_bytes(int64_t n_boxes);
int pgnn_nms_boxes_3d(const int32_t *class_labels, const float *boxes_3d,
                      const float *scores, const int32_t *attributes,
                      int64_t n_boxes, double overlapped_thres, int32_t mode,
                      float appr_factor, int64_t top_k, void *workspace,
                      size_t workspace_bytes, int32_t *out_labels,
                      float *out_boxes, float *out_scores,
                      int32_t *out_attributes, int32_t *out_count,
                      void *stream);
/* overlapped_boxes_3d_fast_poly(single_box, box_list) on (x,y,z,l,h,w,yaw)
 * boxes (nms.py:64-88 after boxes_3d_to_corners :9-27); appr_factor > 0 applies
 * the integer corner rounding of nms.py:115.  overlap [n_boxes] float64. */
int pgnn_overlapped_boxes_3d(const float *single_box, const float *boxes_3d,
                             int64_t n_boxes, float appr_factor,
                             double *overlap, void *stream);
/* overlapped_boxes_3d(single_box, box_list) (nms.py:29-62), the cv2.fillPoly
 * raster overlap random_box_shift calls under every shipped train config
 * (preprocess.py:281-301): integer corner arrays [8,3] / [n_boxes,8,3] int32
 * (np.int32(appr_factor * boxes_3d_to_corners(.))), device pointers; overlap
 * [n_boxes] float64 = np.float32(intersection) / (union - intersection) with
 * pixel counts identical to cv2.fillPoly(LINE_8) + cv2.countNonZero on the
 * (z extent) x (x extent) buffers the reference allocates (OpenCV 4.2
 * drawing.cpp semantics: Bresenham outline after clipLine + 16.16 fixed-point
 * scan-line fill), evaluated in closed form per image row. */
int pgnn_overlapped_boxes_3d_raster(const int32_t *single_box_corners,
                                    const int32_t *box_corners, int64_t n_boxes,
                                    double *overlap, void *stream);

/* ---- KITTI frame ingest (the step right before the
 * path; dataset/kitti_dataset.py:587-609, 998-1006, 1036-1052, 666-689,
 * 990-996 = get_cam_points_in_image[_with_rgb] without the file reads).
 * velo_points [n,4] float32 (x,y,z,reflectance; the .bin layout) on the device;
 * velo_to_cam_3x4 (float32) and cam_to_image_3x3 (float64 = P2[:, :3]) are
 * HOST pointers, copied into the launch.  A point is kept when its camera-frame
 * z > 0.1 and its projection lies strictly inside (0,width) x (0,height);
 * kept points come out in scan order.  out_xyz [capacity,3]; out_attr
 * [capacity,attr_dim]: attr_dim 1 = reflectance, 4 = reflectance + r,g,b
 * sampled from image_bgr ([rows,cols,3] uint8, the cv2.imread layout; may be
 * null -> zeros).  *out_count (device) = number kept (also beyond capacity). */
/* ---- training targets (dataset/kitti_dataset.py
 * :143-162 sel_xyz_in_box3d, :1132-1284 assign_classaware_*_label_to_points;
 * train.py:100-130).  label_records [n_records,24] float64 on the device, one
 * row per ground-truth box in file order: normals[9] (rows wx,wy,wz), lower[3],
 * upper[3] (box3d_to_normals, :118-141, evaluated on the host), action
 * (0 = skip, 1 = object: class + box + valid 1, 2 = class only: valid 0),
 * class value, box[7] = (x3d,y3d,z3d,length,height,width,yaw wrapped into
 * (-pi/4, 3pi/4]).  A vertex strictly inside several boxes keeps what the
 * last one wrote, like the reference's slice assignments.  Outputs (each
 * nullable): cls_labels [n] int32 (0 = background), boxes_3d [n,7] float64,
 * valid_boxes [n] float32, owner [n] int32 = index of the last box containing
 * the vertex or -1 (with one action-1 record: the sel_xyz_in_box3d mask). */
int pgnn_assign_box_labels(const float *xyz, int64_t n_points,
                           const double *label_records, int32_t n_records,
                           int32_t *cls_labels, double *boxes_3d,
                           float *valid_boxes, int32_t *owner, void *stream);
/* Float64 vertices (train.py:100-118 passes the float64 vertex_coord_list of
 * the augmented cloud): np.matmul(xyz_f64, normals.T) on the exact values. */
int pgnn_assign_box_labels_f64(const double *xyz, int64_t n_points,
                               const double *label_records, int32_t n_records,
                               int32_t *cls_labels, double *boxes_3d,
                               float *valid_boxes, int32_t *owner,
                               void *stream);
/* pgnn_box_encode_f32 evaluated in float64 on float64 boxes and a float64
 * class table, rounded to float32 once -- what train.py:120-130 computes
 * (`box_encoding_fn(cls_labels, xyz, boxes_3d_f64, label_map).astype(f32)`). */
int pgnn_box_encode_f64(const int32_t *cls_labels, const float *xyz,
                        const double *boxes, const double *class_table,
                        int32_t n_table, int64_t n_rows, int32_t boxes_per_row,
                        float *encoded, void *stream);
/* ... with float64 vertices as well (train.py:120-122 in the training path). */
int pgnn_box_encode_f64_xyz64(const int32_t *cls_labels, const double *xyz,
                              const double *boxes, const double *class_table,
                              int32_t n_table, int64_t n_rows,
                              int32_t boxes_per_row, float *encoded,
                              void *stream);
/* pgnn_box_encode_canonical_f32 the same way: box_encoding.py:301-343 in
 * float64 on float64 boxes, rounded to float32 once (train.py:120-130 under
 * box_encoding_method 'classaware_all_class_box_canonical_encoding'). */
int pgnn_box_encode_canonical_f64(const int32_t *cls_labels, const float *xyz,
                                  const double *boxes,
                                  const double *class_table, int32_t n_table,
                                  int64_t n_rows, int32_t boxes_per_row,
                                  float *encoded, void *stream);
/* ... with float64 vertices (box_encoding.py:301-343 on train.py:120-122's
 * float64 vertex coordinates). */
int pgnn_box_encode_canonical_f64_xyz64(const int32_t *cls_labels,
                                        const double *xyz, const double *boxes,
                                        const double *class_table,
                                        int32_t n_table, int64_t n_rows,
                                        int32_t boxes_per_row, float *encoded,
                                        void *stream);

/* Point-wise parts of the training augmentations (models/preprocess.py:44-78
 * random_rotation_all / random_flip_all, :239-326 random_box_shift) on a
 * float64 [n,3] device buffer (the reference's cloud is float64 from the first
 * `xyz.dot(R.T)` until train.py:124).  rot_3x3 / shift_3 / box_record_24 are
 * HOST pointers.  pgnn_points_affine_f64: xyz <- xyz @ rot^T + shift for the
 * points with select[i] != 0 (select null: all; rot null: identity).
 * pgnn_points_in_box_f64: inside[i] (nullable) = 1 when point i is strictly
 * inside the box record (layout of pgnn_assign_box_labels), *count (nullable,
 * device) = number of inside points with exclude[i] == 0 (exclude nullable). */
int pgnn_points_affine_f64(double *xyz, int64_t n_points, const double *rot_3x3,
                           const double *shift_3, const int32_t *select,
                           void *stream);
int pgnn_points_in_box_f64(const double *xyz, int64_t n_points,
                           const double *box_record_24, const int32_t *exclude,
                           int32_t *inside, int32_t *count, void *stream);

/* The union mask of remove_background / dilute_background
 * (models/preprocess.py:420-421, :359-360: `mask += sel_xyz_in_box3d(...)` over
 * the selected labels).  box_records is a DEVICE array of n_boxes records of 24
 * doubles (layout and strict predicate of pgnn_points_in_box_f64; `action` is
 * not looked at).  inside[i] (nullable) = 1 when point i is strictly inside any
 * of the boxes and exclude[i] == 0 (exclude nullable; with one record it gives
 * the `new_mask & ~mask` of random_box_global_rotation, :211-213), else 0;
 * *count (nullable, device) = the number of such points.  n_boxes == 0: all
 * zeros.  n_points == 0: *count = 0, nothing else.  No host synchronisation. */
int pgnn_points_in_boxes_f64(const double *xyz, int64_t n_points,
                             const double *box_records, int32_t n_boxes,
                             const int32_t *exclude, int32_t *inside,
                             int32_t *count, void *stream);

/* Order-preserving compaction of the float64 cloud and its attributes: the
 * `xyz[mask]` / `attr[mask]` of random_drop (models/preprocess.py:27),
 * random_box_global_rotation (:220-221), remove_background (:427-428) and
 * dilute_background (:367-371).  Point i is kept when
 *   (keep == NULL || keep[i] != 0) && (drop == NULL || drop[i] == 0)
 * (int32 device masks).  attr is float32 [n_points, attr_dim] with attr_dim in
 * 0..4, or NULL (then out_attr is not touched).  The kept rows go, in their
 * original order, to out_xyz [capacity,3] / out_attr [capacity,attr_dim];
 * *out_count (device) = the number of kept points also when that exceeds
 * `capacity`, and nothing is written past `capacity` rows.  n_points == 0:
 * *out_count = 0.  n_points < 2^31.  Two launches around an exclusive scan of
 * the per-block counts (the shape of pgnn_kitti_cam_points_in_image); no host
 * synchronisation.  Workspace: pgnn_points_compact_workspace_bytes(n_points). */
size_t pgnn_points_compact_workspace_bytes(int64_t n_points);
int pgnn_points_compact_f64(const double *xyz, const float *attr,
                            int32_t attr_dim, int64_t n_points,
                            const int32_t *keep, const int32_t *drop,
                            void *workspace, size_t workspace_bytes,
                            double *out_xyz, float *out_attr, int64_t capacity,
                            int32_t *out_count, void *stream);

/* crop_aug object pasting: the trial search of parser_without_collision
 * (models/crop_aug.py:75-186) for one frame in ONE launch of one workgroup.
 * Device inputs: the float64 base cloud base_xyz [n_base,3]; the sampled
 * objects' points sample_xyz [n_sample_points,3] with sample_offsets
 * [n_samples+1] (0 = off[0] <= ... <= off[S] = n_sample_points; anything else
 * is reported, see below, and nothing is written); their boxes sample_boxes
 * [n_samples,7] (x,y,z,l,h,w,yaw); the labels' integer corner grids
 * label_corners [n_labels,8,3] = np.int32(appr_factor *
 * boxes_3d_to_corners(.)) (:87-92; not read in 'point' mode); and the draw
 * table draws [n_samples*max_trails,3] = (delta_yaw, cos, sin) in the order
 * NumPy's stream yields them.  expand_factor_3 is a HOST pointer.
 * overlap_mode: 0 'box', 1 'point', 2 'box_and_point' (:131-164).
 *
 * Samples and trials are walked in the reference's order; draw k goes to the
 * k-th trial actually run (one flat cursor).  A trial turns the centre by the
 * drawn yaw (:104-113); with auto_box_height it takes the largest y among the
 * alive points strictly inside the box's y/z normals (sel_xyz_in_box2d,
 * kitti_dataset.py:164-182) as the ground, y3d += ground - y3d (:114-127; no
 * such point: the trial is spent under must_have_ground, else no lift); the
 * box test is overlapped_boxes_3d_fast_poly (nms.py:64-88) of the trial's
 * integer corner grid against every label and every box accepted so far, all
 * `< max_overlap_rate`; the point test is `count of alive points strictly
 * inside the expanded box < max_overlap_num_allowed`.  Accepted: those points
 * die, the sample's points come alive turned by the drawn yaw (and lifted).
 *
 * Outputs (device): work_xyz [n_sample_points+n_base,3] = [block of sample
 * S-1, ..., block of sample 0, base cloud] with alive [.] int32 flags --
 * pgnn_points_compact_f64 with keep = alive yields the reference's cloud, each
 * accepted object in front of what was there (:172-175); record
 * [3*n_samples+2] float64 = per sample (accepted, index of the accepting draw
 * or -1, ground height or NaN), then the draws consumed and the number of alive
 * rows (both -1 for a bad offset table).  cand_xyz [rows,3] / cand_idx [rows]
 * are scratch of the same row count: per sample, the alive rows whose distance
 * from the y axis is within the footprint's half diagonal of the centre's --
 * the only ones a trial's box can hold, since a trial turns the box about that
 * axis -- are gathered once and the trials read those.  Float64 throughout, no contraction;
 * max and counts are order-independent.  Every loop is bounded by n_samples *
 * (max_trails + 1) * ceil(rows / 512); one workgroup, so none waits for another.
 * PGNN_E_UNSUPPORTED: n_labels + n_samples > 256 outside 'point' mode (the
 * boxes live in LDS), 2^30 rows or draws.  No host synchronisation. */
int pgnn_crop_aug_place(const double *base_xyz, int64_t n_base,
                        const double *sample_xyz,
                        const int32_t *sample_offsets, int32_t n_samples,
                        int64_t n_sample_points, const double *sample_boxes,
                        const int32_t *label_corners, int32_t n_labels,
                        const double *draws, int32_t max_trails,
                        int32_t overlap_mode, int32_t auto_box_height,
                        int32_t must_have_ground, double max_overlap_rate,
                        double appr_factor, double max_overlap_num_allowed,
                        const double *expand_factor_3, double *work_xyz,
                        int32_t *alive, double *cand_xyz, int32_t *cand_idx,
                        double *record, void *stream);

/* Streaming classification metrics of the training / evaluation loops
 * (train.py:301-368, eval.py:176-245): per class tf.metrics.recall and
 * tf.metrics.precision of argmax(probs) against the labels, and
 * tf.metrics.auc(labels == c, probs[:, c], num_thresholds, curve='PR',
 * summation_method='careful_interpolation').  `state` is a caller-owned device
 * buffer of pgnn_metrics_state_bytes() bytes, zeroed by the caller to reset
 * (the reference re-initialises its local variables per epoch); it holds int64
 * counters only, so states of several ranks add up with one integer
 * all-reduce.  pgnn_metrics_update folds one batch in; pgnn_metrics_compute
 * writes out[c*3 + {0,1,2}] = recall, precision, PR-AUC of class c (float32
 * arithmetic as TensorFlow's). */
size_t pgnn_metrics_state_bytes(int32_t n_classes, int32_t n_thresholds);
int pgnn_metrics_update(const float *probs, int64_t ld_probs,
                        const int32_t *labels, int64_t n_rows,
                        int32_t n_classes, int32_t n_thresholds, void *state,
                        void *stream);
int pgnn_metrics_compute(const void *state, int32_t n_classes,
                         int32_t n_thresholds, float *out, void *stream);

/* KITTI object-detection average precision of a frame set: the 2D box, the
 * bird's-eye box and the 3D box, for Car / Pedestrian / Cyclist at the easy /
 * moderate / hard difficulties, with 11- and 40-point interpolation.  The
 * protocol (constants, overlaps, cleaning, matching, thresholds, curve) is
 * stated in full in DESIGN.md section 9.5; these entries implement exactly
 * that text, in float64.  The reference has no counterpart: its README hands
 * the result files to an external evaluation program.
 *
 * Boxes are rows of PGNN_KITTI_ROW doubles,
 *   xmin ymin xmax ymax  height width length  x3d y3d z3d  yaw
 *   truncation occlusion score
 * (score is read for detections only, truncation and occlusion for ground
 * truths only), with one int32 name code per box: 0 Car, 1 Pedestrian,
 * 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else.  Frame f
 * owns the ground truths gt_offsets[f] .. gt_offsets[f+1]-1 and the detections
 * det_offsets[f] .. det_offsets[f+1]-1, in file order.
 *
 * gt_offsets / det_offsets: HOST arrays of n_frames + 1 int32, starting at 0
 * and ascending; the entries check them, derive every size from them and copy
 * them to the workspace in stream order (keep them alive until the stream has
 * passed the call).  Everything else is a device pointer; box and name
 * pointers may be NULL when their count is 0.
 *
 * Caps, per frame: PGNN_KITTI_MAX_DET detections (the assigned set is a bit
 * mask of 16 64-bit words per lane in LDS) and PGNN_KITTI_MAX_GT ground
 * truths; at most PGNN_KITTI_MAX_FRAMES frames.  Beyond a cap:
 * PGNN_E_UNSUPPORTED with the frame and its counts in pgnn_last_error, nothing
 * launched and nothing written.  Other argument errors: PGNN_E_INVALID;
 * workspace too small: PGNN_E_WORKSPACE; both before any HIP call.
 *
 * pgnn_kitti_eval_workspace_bytes: bytes for n_frames frames holding n_gt
 * ground truths, n_det detections and n_pairs = sum over frames of (ground
 * truths * detections) pairs; 0 for arguments out of range.
 *
 * pgnn_kitti_pair_overlaps: overlaps[m * n_pairs + pair_off[f] + i * nd_f + j]
 * for ground truth i and detection j of frame f (pair_off[f] = the pairs of
 * the frames before f): m = 0 the 2D, 1 the BEV, 2 the 3D union overlap, 3 the
 * 2D detection-criterion overlap where ground truth i is a DontCare, else 0.
 * pgnn_kitti_eval computes the same values once, into its workspace, and every
 * comparison of the matching reads them from there.
 *
 * pgnn_kitti_eval: the number of launches does not depend on n_frames, nothing
 * is read back, and the outputs are complete when `stream` has passed the
 * call.  Combination index = (metric * 3 + class) * 3 + difficulty, metric
 * 0 = 2D, 1 = BEV, 2 = 3D (PGNN_KITTI_COMBOS = 27 combinations):
 *   precision, recall  [27][41] float64 (precision after the running maximum;
 *                      entries past n_thresholds, and a quotient whose
 *                      denominator is 0, are 0)
 *   counters           [27][41][3] int64: tp, fp, fn at each threshold
 *   thresholds         [27][41] float64, n_thresholds [27] int32
 *   n_gt               [27] int64
 *   ap_r11, ap_r40     [27] float64, in [0, 1]
 * The counters are sums of integers, so the outputs are the same bits on
 * every run and every stream.
 *
 * pgnn_kitti_eval_ex: pgnn_kitti_eval with two additions (DESIGN.md section
 * 9.5, "Orientation" and "Overlap table").
 *   min_overlap   HOST pointer to 9 doubles [metric][class], the bound of
 *                 `overlap > MIN_OVERLAP` (the DontCare step of the 2D metric
 *                 reads the 2D row); NULL = the official table, 0.7 / 0.5 / 0.5
 *                 for every metric, which is what pgnn_kitti_eval uses.  Every
 *                 entry must be finite and in [0, 1]: else PGNN_E_INVALID.
 *   gt_alpha, det_alpha   device float64, one observation angle per box, in
 *                 the order of the box rows.  Both NULL: no orientation, the
 *                 four outputs below are not touched (and may be NULL), and
 *                 the launches are those of pgnn_kitti_eval.  Exactly one
 *                 NULL: PGNN_E_INVALID.
 *   similarity    [9][41] float64, the 2D metric's [class][difficulty]: the
 *                 sum over the true positives at each threshold of
 *                 (1 + cos(alpha_gt - alpha_det)) / 2
 *   orientation   [9][41] float64: similarity / (tp + fp) (0 past n_thresholds
 *                 and for an empty denominator), after the running maximum
 *   aos_r11, aos_r40   [9] float64, the sums of ap_r11 / ap_r40 over orientation
 * Orientation changes no matching decision: every other output is the same
 * bits with and without it.  The similarity sums use no floating-point
 * atomics (each wave of the second pass has its own slot, added in ascending
 * order), so they too are the same bits on every run and every stream.
 * pgnn_kitti_eval_ex_workspace_bytes: as pgnn_kitti_eval_workspace_bytes;
 * with_aos != 0 adds a fifth pair plane and the wave slots (at most
 * 9 * 1024 * 41 doubles).
 *
 * pgnn_kitti_pair_orientation: sim[pair_off[f] + i * nd_f + j] =
 * (1 + cos(gt_alpha[i] - det_alpha[j])) / 2 where the 2D union overlap of the
 * pair is > 0, else 0: the plane the evaluation with orientation computes once
 * into its workspace, in the layout of one plane of pgnn_kitti_pair_overlaps
 * (and with its workspace).                                                  */
#define PGNN_KITTI_ROW 14
#define PGNN_KITTI_COMBOS 27
#define PGNN_KITTI_SAMPLE_PTS 41
#define PGNN_KITTI_MAX_DET 1024
#define PGNN_KITTI_MAX_GT 1024
#define PGNN_KITTI_MAX_FRAMES (1 << 24)
size_t pgnn_kitti_eval_workspace_bytes(int64_t n_frames, int64_t n_gt,
                                       int64_t n_det, int64_t n_pairs);
int pgnn_kitti_pair_overlaps(const int32_t *gt_offsets /* host */,
                             const int32_t *det_offsets /* host */,
                             int64_t n_frames, const double *gt_boxes,
                             const int32_t *gt_names, const double *det_boxes,
                             void *workspace, size_t workspace_bytes,
                             double *overlaps, void *stream);
int pgnn_kitti_eval(const int32_t *gt_offsets /* host */,
                    const int32_t *det_offsets /* host */, int64_t n_frames,
                    const double *gt_boxes, const int32_t *gt_names,
                    const double *det_boxes, const int32_t *det_names,
                    void *workspace, size_t workspace_bytes, double *precision,
                    double *recall, int64_t *counters, double *thresholds,
                    int32_t *n_thresholds, int64_t *n_gt, double *ap_r11,
                    double *ap_r40, void *stream);
size_t pgnn_kitti_eval_ex_workspace_bytes(int64_t n_frames, int64_t n_gt,
                                          int64_t n_det, int64_t n_pairs,
                                          int32_t with_aos);
int pgnn_kitti_eval_ex(const int32_t *gt_offsets /* host */,
                       const int32_t *det_offsets /* host */, int64_t n_frames,
                       const double *gt_boxes, const int32_t *gt_names,
                       const double *det_boxes, const int32_t *det_names,
                       void *workspace, size_t workspace_bytes,
                       double *precision, double *recall, int64_t *counters,
                       double *thresholds, int32_t *n_thresholds, int64_t *n_gt,
                       double *ap_r11, double *ap_r40, const double *gt_alpha,
                       const double *det_alpha,
                       const double *min_overlap /* host */, double *similarity,
                       double *orientation, double *aos_r11, double *aos_r40,
                       void *stream);
int pgnn_kitti_pair_orientation(const int32_t *gt_offsets /* host */,
                                const int32_t *det_offsets /* host */,
                                int64_t n_frames, const double *gt_boxes,
                                const double *det_boxes, const double *gt_alpha,
                                const double *det_alpha, void *workspace,
                                size_t workspace_bytes, double *sim,
                                void *stream);

/* pgnn_kitti_match: what the matching of ONE (metric, class, difficulty)
 * decides at ONE score threshold, per box, for a whole frame set (DESIGN.md
 * section 9.13).  Inputs, caps, error codes and argument checks are those of
 * pgnn_kitti_eval_ex; also PGNN_E_INVALID: metric, cls or difficulty outside
 * 0..2, a score_threshold that is not finite, a loc_floor that is not in
 * [0, 1].  The cleaning flags and the overlaps come from the evaluation's own
 * kernels, the matching is section 9.5's with compute_fp, at score_threshold,
 * with min_overlap[metric][cls] (NULL = the official table).  The number of
 * launches does not depend on n_frames and nothing is read back.
 *
 *   det_outcome  [n_det] int32, a PGNN_KITTI_DET_* code; the rules are tested
 *                in the order of the codes (idj = the detection's cleaning
 *                result, ig = a ground truth's):
 *     OTHER            idj == -1
 *     BELOW            score < score_threshold
 *     TP               assigned, ig == 0 and idj == 0
 *     MATCHED_IGNORED  assigned, ig == 1 or idj == 1
 *     IGNORED_SMALL    idj == 1, not assigned
 *     DONTCARE         2D metric only: absorbed by a DontCare row (the first
 *                      row, in file order, whose detection-criterion overlap
 *                      with it is > min_overlap)
 *     FP_*             a false positive.  b = its largest overlap with a
 *                      ground truth of ig >= 0, x = with one of ig == -1 that
 *                      is no DontCare (smallest index on ties; an overlap of
 *                      0 names no ground truth):
 *       FP_DUPLICATE     b > min_overlap (that ground truth went elsewhere)
 *       FP_CONFUSION     else x >= loc_floor and x > b
 *       FP_LOCALISATION  else b >= loc_floor
 *       FP_BACKGROUND    else
 *   gt_outcome   [n_gt] int32, a PGNN_KITTI_GT_* code:
 *     OTHER            ig == -1
 *     IGNORED / IGNORED_MATCHED   ig == 1, not assigned / assigned
 *     TP / MATCHED_SMALL          ig == 0, assigned, idj == 0 / idj == 1
 *     FN_LOW_SCORE     not assigned; a detection of idj != -1 and score <
 *                      score_threshold overlaps it by more than min_overlap
 *     FN_LOCALISATION  else a detection of idj == 0 and score >=
 *                      score_threshold has loc_floor <= overlap <= min_overlap
 *     FN_MISSED        else
 *   gt_partner, det_partner   int32, an index within the frame or -1: the
 *                assigned pair (TP, MATCHED_IGNORED, IGNORED_MATCHED,
 *                MATCHED_SMALL); the ground truth of b (FP_DUPLICATE,
 *                FP_LOCALISATION) or of x (FP_CONFUSION); the absorbing row
 *                (DONTCARE); for FN_LOW_SCORE / FN_LOCALISATION the detection
 *                of the largest overlap among those the rule names (smallest
 *                index on ties)
 *   det_overlap  [n_det] float64: the overlap with the partner, a copy of the
 *                overlap table's entry (DONTCARE: the detection-criterion
 *                overlap); 0 without a partner
 *   totals       [PGNN_KITTI_MATCH_TOTALS] int64: boxes per detection code,
 *                then per ground-truth code
 * Every output is an integer or a copy: the same bits on every run and every
 * stream.  Outcome pointers may be NULL when their count is 0.              */
#define PGNN_KITTI_DET_OTHER 0
#define PGNN_KITTI_DET_BELOW 1
#define PGNN_KITTI_DET_TP 2
#define PGNN_KITTI_DET_MATCHED_IGNORED 3
#define PGNN_KITTI_DET_IGNORED_SMALL 4
#define PGNN_KITTI_DET_DONTCARE 5
#define PGNN_KITTI_DET_FP_DUPLICATE 6
#define PGNN_KITTI_DET_FP_CONFUSION 7
#define PGNN_KITTI_DET_FP_LOCALISATION 8
#define PGNN_KITTI_DET_FP_BACKGROUND 9
#define PGNN_KITTI_DET_CODES 10
#define PGNN_KITTI_GT_OTHER 0
#define PGNN_KITTI_GT_IGNORED 1
#define PGNN_KITTI_GT_IGNORED_MATCHED 2
#define PGNN_KITTI_GT_TP 3
#define PGNN_KITTI_GT_MATCHED_SMALL 4
#define PGNN_KITTI_GT_FN_LOW_SCORE 5
#define PGNN_KITTI_GT_FN_LOCALISATION 6
#define PGNN_KITTI_GT_FN_MISSED 7
#define PGNN_KITTI_GT_CODES 8
#define PGNN_KITTI_MATCH_TOTALS (PGNN_KITTI_DET_CODES + PGNN_KITTI_GT_CODES)
size_t pgnn_kitti_match_workspace_bytes(int64_t n_frames, int64_t n_gt,
                                        int64_t n_det, int64_t n_pairs);
int pgnn_kitti_match(const int32_t *gt_offsets /* host */,
                     const int32_t *det_offsets /* host */, int64_t n_frames,
                     const double *gt_boxes, const int32_t *gt_names,
                     const double *det_boxes, const int32_t *det_names,
                     const double *min_overlap /* host */, int32_t metric,
                     int32_t cls, int32_t difficulty, double score_threshold,
                     double loc_floor, void *workspace, size_t workspace_bytes,
                     int32_t *gt_outcome, int32_t *gt_partner,
                     int32_t *det_outcome, int32_t *det_partner,
                     double *det_overlap, int64_t *totals, void *stream);

size_t pgnn_kitti_ingest_workspace_bytes(int64_t n_points);
int pgnn_kitti_cam_points_in_image(
    const float *velo_points, int64_t n_points, const float *velo_to_cam_3x4,
    const double *cam_to_image_3x3, double image_width, double image_height,
    const uint8_t *image_bgr, int64_t image_rows, int64_t image_cols,
    void *workspace, size_t workspace_bytes, float *out_xyz, float *out_attr,
    int32_t attr_dim, int64_t capacity, int32_t *out_count, void *stream);

/* ---- voxel-average down-sampling of a frame (dataset/kitti_dataset.py:16-48
 * downsample_by_average_voxel; the `downsample_by_voxel_size` key of every
 * config, passed to the frame fetch at run.py:210-211, train.py:80, eval.py:70).
 * xyz [n,3] float32 and attr [n,attr_dim] float32 (nullable; attr_dim 0..4) on
 * the device.  kitti_dataset.py:24-28: idx = ((xyz - amin(xyz)) // voxel_size)
 * .astype(int32) with NumPy's float32 floor_divide (voxel_size, a double here,
 * is applied as NumPy applies a Python float to a float32 array: in float32);
 * :29-30 key = ix + iy*dim_x + iz*dim_y*dim_x in WRAPPING int32, rows come out
 * in ascending signed key; :31-38 each voxel's rows are summed sequentially in
 * float32 and divided by the int64 count, so the result is float64:
 * out_xyz [capacity,3], out_attr [capacity,attr_dim], out_lens [capacity]
 * (nullable: points per voxel).  The reference's argsort is not stable, so for
 * voxels of three or more points its summation order is the sort
 * implementation's; here it is DEFINED: ascending original index.
 * n_dev (nullable, device int32): the point count when only the device knows
 * it; n_points is then the capacity everything is sized for and
 * min(*n_dev, n_points) points are read.  *out_count (device) = number of
 * voxels (also beyond capacity).  Enqueued on `stream`, no host read.
 * n_points == 0 is PGNN_E_INVALID (the reference raises on np.amax of an
 * empty array), as are voxel_size <= 0 or not finite and attr_dim > 4. */
size_t pgnn_voxel_average_workspace_bytes(int64_t n_points, int32_t attr_dim);
int pgnn_voxel_average_f32(const float *xyz, const float *attr,
                           int32_t attr_dim, int64_t n_points,
                           const int32_t *n_dev, double voxel_size,
                           void *workspace, size_t workspace_bytes,
                           double *out_xyz, double *out_attr, int32_t *out_lens,
                           int64_t capacity, int32_t *out_count, void *stream);
/* get_cam_points_in_image[_with_rgb] with a voxel size (kitti_dataset.py
 * :612-628 get_cam_points = :998-1006 velo_points_to_cam, then the
 * down-sampling above on xyz and the reflectance; :666-716 front mask z > 0.1,
 * :1036-1052 float64 projection, strict image crop, :985-996 colour lookup --
 * all on the FLOAT64 voxel rows, the voxel count handed on in device memory).
 * Arguments as pgnn_kitti_cam_points_in_image; out_xyz [capacity,3] and
 * out_attr [capacity,attr_dim] are float64 (np.hstack([attr, rgb]) of a
 * float64 and a float32 array is float64); kept rows are in voxel-key order. */
size_t pgnn_kitti_cam_points_voxel_in_image_workspace_bytes(int64_t n_points);
int pgnn_kitti_cam_points_voxel_in_image(
    const float *velo_points, int64_t n_points, const float *velo_to_cam_3x4,
    const double *cam_to_image_3x3, double image_width, double image_height,
    const uint8_t *image_bgr, int64_t image_rows, int64_t image_cols,
    double voxel_size, void *workspace, size_t workspace_bytes,
    double *out_xyz, double *out_attr, int32_t attr_dim, int64_t capacity,
    int32_t *out_count, void *stream);

/* ---- beam decimation (scripts/point_cloud_downsample.py:19-53: the inputs of
 * the sparse-LiDAR experiment, every rate-th scanning line of a scan kept).
 * The script clusters the elevation cosine of every point into 64 beams with
 * an UNSEEDED KMeans, so it has no output to match; the clustering here is
 * DEFINED, a function of the input bits only.
 * velo_points [n,4] float32 rows (x, y, z, reflectance) on the device.
 *   cosine (:22-25, :29)  norm = sqrt_f32((x*x + y*y) + z*z), every operation
 *     float32, round to nearest, no FMA, the root correctly rounded;
 *     cos = (double)z / (double)norm -- bit for bit the script's NumPy value.
 *     A row is INVALID when norm == 0 or x, y or z is not finite: it takes no
 *     part in the clustering and is never kept (the script's KMeans raises).
 *   quantisation  q = rint(cos * 2^30), ties to even; all clustering runs on
 *     q, sums are exact integers.  s_0 <= ... <= s_{v-1}: the q of the v valid
 *     rows, sorted; S_i their exact prefix sums.
 *   initial centres (farthest-first)  C = {s_0}; n_beams - 1 times:
 *     d_i = min over c in C of |s_i - c|, the SMALLEST i of maximal d_i joins
 *     C; a maximal d_i of 0 is status 2.  c_0 <= ... = sorted(C) as float64.
 *   Lloyd passes  m_j = c_{j-1} + c_j; hi_j = #{i : 2 s_i <= m_{j+1}} for
 *     j < n_beams - 1, hi_{n_beams-1} = v; cluster j = [hi_{j-1}, hi_j) with
 *     hi_{-1} = 0 (a point on a midpoint goes to the lower cluster);
 *     c_j = (double)(S[hi_j] - S[hi_{j-1}]) / (double)(hi_j - hi_{j-1}), an
 *     empty cluster keeps c_j.  A pass whose every hi_j equals the previous
 *     pass's ends the loop (status 0; the first pass has no previous one);
 *     max_iter passes without that is status 3, the centres still valid.
 *   centers [n_beams] = c_j * 2^-30, ascending.
 *   info [4] = {v, passes made, status, 0}; status 0 ok, 1: v < n_beams,
 *     2: fewer than n_beams distinct q, 3: max_iter reached.  With status 1 or
 *     2 centers are 0, passes 0, and pgnn_beam_select keeps nothing.
 * pgnn_beam_select (:27-35, :50): ext = [-1, centers, +1]; for i = 0, rate,
 *   2 rate, ... < n_beams a valid row is kept when (ext[i] + ext[i+1]) / 2 <
 *   cos < (ext[i+1] + ext[i+2]) / 2 in float64 with the unquantised cos --
 *   strict, as in the script: a row on a bound is dropped, even at rate 1, and
 *   the outer bounds are (-1 + c_0) / 2 and (c_last + 1) / 2.  Kept rows are
 *   copied bit for bit (all four floats) in their original order to
 *   out_points [n_points,4]; *out_count (device) is their number.  info
 *   (nullable, device): the info of pgnn_beam_centers.
 * One workspace size serves both entries.  Both are enqueued on `stream`, no
 * host read.  PGNN_E_INVALID: n_beams outside 2..64, rate < 1, max_iter < 1,
 * null pointers.  n_points == 0 gives status 1 and a count of 0. */
size_t pgnn_beam_workspace_bytes(int64_t n_points);
int pgnn_beam_centers(const float *velo_points, int64_t n_points,
                      int32_t n_beams, int32_t max_iter, void *workspace,
                      size_t workspace_bytes, double *centers /* [n_beams] */,
                      int32_t *info /* [4] */, void *stream);
int pgnn_beam_select(const float *velo_points, int64_t n_points,
                     const double *centers, int32_t n_beams, int32_t rate,
                     const int32_t *info, void *workspace,
                     size_t workspace_bytes, float *out_points,
                     int32_t *out_count, void *stream);

/* ---- farthest-point sampling (dataset/kitti_dataset.py:630-641:
 * KittiDataset.farthest_first with its helper calc_distances).
 * For one cloud pts [n, 3] (float32, or _f64 float64), a start index s and a
 * count k, a pure function of the input bits:
 *   d_j    = (dx*dx + dy*dy) + dz*dz with dx = p_s.x - p_j.x, ...: float64, one
 *            rounding per operation, nothing contracted; float32 coordinates
 *            are widened first (what :631 computes on a [n, 3] array)
 *   pick_0 = s
 *   pick_i = smallest j with d_j == max(d)               (np.argmax, :638)
 *   d_j    = min(d_j, dist(pick_i, j))                   (np.minimum, :639)
 * k > n, duplicate points and all-equal clouds follow from these rules: once
 * max(d) == 0 every later pick is index 0, and the kernel stops iterating there
 * and fills the tail.  num_distinct = the smallest i >= 1 whose round found
 * max(d) == 0, or k when there is none: picks [0, num_distinct) are pairwise
 * non-coincident.
 * Segmented form: offsets int32 [n_segments + 1] (device) over the concatenated
 * cloud, start int32 [n_segments] (device, indices LOCAL to the segment), one
 * k.  out_idx int32 [n_segments, k] local indices, out_xyz (nullable)
 * [n_segments, k, 3] the picked rows copied bit for bit in the input dtype,
 * num_distinct int32 [n_segments].  An empty segment writes -1, zero rows and
 * num_distinct 0.  offsets == NULL with n_segments == 1 is the single cloud
 * [0, n_points).  k == 0 or n_points == 0 write nothing but num_distinct.
 * A start index outside its segment is the caller's error (the host cannot see
 * it here); the kernel clamps it into the segment and never reads out of
 * range.  Rows with a non-finite coordinate are outside the contract, as for
 * the reference; the kernel terminates and every index it writes lies in
 * [0, n).
 * One workgroup of PGNN_FPS_BLOCK threads per segment, persistent over the k
 * rounds, workgroup barriers only.  A segment of at most PGNN_FPS_RESIDENT
 * (float32) / PGNN_FPS_RESIDENT_F64 (float64) points keeps coordinates and
 * running distances on chip (registers, part of the distances in LDS); a
 * larger one streams its coordinates every round and keeps the distances in
 * the workspace (pgnn_farthest_first_workspace_bytes: 8 bytes per point of a
 * cloud above the smaller limit, else 0).  No host read, one launch.
 * PGNN_E_INVALID: null pointer, negative size, offsets == NULL with
 * n_segments != 1, n_points >= 2^31. */
#define PGNN_FPS_BLOCK 512
#define PGNN_FPS_RESIDENT (40 * PGNN_FPS_BLOCK)
#define PGNN_FPS_RESIDENT_F64 (20 * PGNN_FPS_BLOCK)
size_t pgnn_farthest_first_workspace_bytes(int64_t n_points,
                                           int64_t n_segments, int32_t k);
int pgnn_farthest_first(const float *points, const int32_t *offsets,
                        int64_t n_segments, int64_t n_points,
                        const int32_t *start, int32_t k, void *workspace,
                        size_t workspace_bytes, int32_t *out_idx,
                        float *out_xyz, int32_t *num_distinct, void *stream);
int pgnn_farthest_first_f64(const double *points, const int32_t *offsets,
                            int64_t n_segments, int64_t n_points,
                            const int32_t *start, int32_t k, void *workspace,
                            size_t workspace_bytes, int32_t *out_idx,
                            double *out_xyz, int32_t *num_distinct,
                            void *stream);

/* ---- rendering: the frame, its boxes and its graph drawn into an image on
 * the device (run.py -l 1|2: :152-175 the open3d window, :328-359 the cloud and
 * the graph edges into the kept vertices, :410-421 cv2.rectangle per detection,
 * :434-535 the box line sets and the camera image; kitti_dataset.py
 * boxes_3d_to_line_set :785-822, vis_draw_2d_box, vis_draw_3d_box, vis_points,
 * vis_graph, vis_point_graph, inspect_points).  There is no display, open3d or
 * cv2 here: the output is a uint8 RGB image [height, width, 3], row-major,
 * origin top left.  Text (cv2.putText) is a pass of its own over a finished
 * image: "text" below.  NOT drawn: the interactive 3D window.  The semantics
 * are integer-exact: every step below is an IEEE float64 + - * / in the order
 * written, a floor, or integer arithmetic.
 *
 * canvas   1 <= width, height <= PGNN_RENDER_MAX_DIM (4096).
 * view     view_m [3][4] and view_d [4] float64 in HOST memory, near float64.
 *   For a point (x, y, z), float32 or float64 (is_f64), widened to float64:
 *     hu = ((m00 x + m01 y) + m02 z) + m03, hv and hw from rows 1 and 2,
 *     depth = ((d0 x + d1 y) + d2 z) + d3.
 *   A point is VISIBLE when hu, hv, hw and depth are finite and hw >= near;
 *   its pixel is u = floor(hu / hw), v = floor(hv / hw), compared as float64
 *   with 0 <= u < width, 0 <= v < height; a point whose pixel is off the
 *   canvas is not drawn.
 * points   (pgnn_render_points) a visible point covers [u, u+p) x [v, v+p)
 *   clipped to the canvas, p = point_size in 1..3.  On each pixel the point
 *   with the smallest float32(depth) wins (-0 and +0 are equal), among equal
 *   depths the smallest index.  n_points < 2^30.
 * segments (pgnn_render_segments) [n, 2, 3]: ends a, b mapped to (hu, hv, hw)
 *   as above.  A non-finite value drops the segment; hw < near at both ends
 *   drops it; hw < near at one end (call it a) clips that end:
 *     t = (near - hw_a) / (hw_b - hw_a), hu_a = hu_a + t (hu_b - hu_a), hv_a
 *     alike, hw_a = near exactly.
 *   Each end's pixel is (floor(hu / hw), floor(hv / hw)); a coordinate with
 *   |value| >= 2^30 (or NaN) drops the segment; the rest is int64.  With
 *   dx = x1 - x0, dy = y1 - y0, N = max(|dx|, |dy|): N = 0 is the one pixel;
 *   if |dx| >= |dy| the pixels are x = x0 + k sgn(dx),
 *   y = y0 + floordiv(2 k dy + N, 2 N) for k = 0..N (floordiv rounds toward
 *   -inf: a midpoint on a half goes up by one), otherwise with x and y
 *   swapped.  Each pixel is stamped with a t x t square at offsets
 *   -floor((t-1)/2) .. floor(t/2) on both axes, t = thickness in 1..3: one
 *   value for all, or thickness_per_segment (device uint8 [n], then
 *   `thickness` is ignored; a value outside 1..3 drops that segment).  Pixels
 *   off the canvas are skipped.  Only the k whose major coordinate lies within
 *   one pixel of the canvas are visited: the work per segment is bounded by
 *   the canvas, not by N.  On each pixel the segment with the LARGEST index
 *   wins, as a later cv2.line overwrites an earlier one.
 * resolve  (pgnn_render_resolve) per pixel the first that applies: the
 *   winning segment's colour, the winning point's colour, the background
 *   (background_image, device uint8 [height, width, 3], or when that is null
 *   background_rgb = r << 16 | g << 8 | b).  Colours are device uint8 [n, 3];
 *   n_*_colors == 1 is one colour for the whole layer, otherwise one row per
 *   primitive (a winner without a row shows the background).
 * The workspace holds one uint64 key per pixel; pgnn_render_clear empties it,
 * pgnn_render_points / pgnn_render_segments may then be called any number of
 * times with the SAME canvas (indices are per call: colours resolve against
 * the last call of each kind), pgnn_render_resolve writes the image.
 * pgnn_render_colorize: i = floor((float64(v) - lo) / (hi - lo) * 255) clamped
 * to 0..255, NaN gives 0; colors [n, 3] = table[i], table device uint8
 * [256, 3].
 * pgnn_render_graph_segments (run.py:341-350, vis_graph): segments [n_edges,
 * 2, 3] float32 = (src_xyz[edges[e][0]], dst_xyz[edges[e][1]]), edges int32
 * [n_edges, 2]; an index outside its array gives a NaN end (the segment is
 * dropped when drawn).  Host-sized only.
 * All entries enqueue on `stream`; none reads back.  PGNN_E_INVALID (nothing
 * enqueued): width or height outside 1..4096, point_size or thickness outside
 * 1..3, near not finite, a null pointer with a non-zero count;
 * PGNN_E_WORKSPACE: workspace_bytes below pgnn_render_workspace_bytes (which
 * is 0 for a canvas out of range).                                          */
#define PGNN_RENDER_MAX_DIM 4096
size_t pgnn_render_workspace_bytes(int32_t width, int32_t height);
int pgnn_render_clear(int32_t width, int32_t height, void *workspace,
                      size_t workspace_bytes, void *stream);
int pgnn_render_points(const void *xyz, int32_t is_f64, int64_t n_points,
                       const double *view_m /* host [12] */,
                       const double *view_d /* host [4] */, double near,
                       int32_t width, int32_t height, int32_t point_size,
                       void *workspace, size_t workspace_bytes, void *stream);
int pgnn_render_segments(const void *segments, int32_t is_f64,
                         int64_t n_segments,
                         const double *view_m /* host [12] */, double near,
                         int32_t width, int32_t height,
                         const uint8_t *thickness_per_segment,
                         int32_t thickness, void *workspace,
                         size_t workspace_bytes, void *stream);
int pgnn_render_resolve(int32_t width, int32_t height, const void *workspace,
                        size_t workspace_bytes, const uint8_t *point_colors,
                        int64_t n_point_colors, const uint8_t *segment_colors,
                        int64_t n_segment_colors,
                        const uint8_t *background_image,
                        uint32_t background_rgb, uint8_t *image, void *stream);
int pgnn_render_colorize(const void *values, int32_t is_f64, int64_t n,
                         double lo, double hi, const uint8_t *table,
                         uint8_t *colors, void *stream);
int pgnn_render_graph_segments(const float *src_xyz, int64_t n_src,
                               const float *dst_xyz, int64_t n_dst,
                               const int32_t *edges, int64_t n_edges,
                               float *segments, void *stream);

/* ---- text: strings of a built-in 5 x 7 font drawn into an image -------------
 * What cv2.putText does for run.py -l 1 (:414-421, 'P | 0.873' beside every
 * detection) and vis_draw_2d_box (kitti_dataset.py:1069-1084, the object's
 * name).  There is no font file here: the font is one table of this library,
 * uint8 [95][7] for the printable ASCII codes 0x20..0x7E (csrc/font5x7.h).  A
 * glyph has 5 columns and 7 rows; a row is a bit mask, bit 4 the leftmost
 * column, bit 0 the rightmost; row 0 is the top.  pgnn_render_font copies the
 * table to HOST memory [95 * 7] (no device needed).  Integer arithmetic only.
 *
 * image    pgnn_render_text draws IN PLACE into a device uint8 [height, width,
 *   3] image, over whatever it holds (the output of pgnn_render_resolve, a
 *   camera picture, one colour).  Canvas as above, 1..PGNN_RENDER_MAX_DIM.
 * inputs   all in DEVICE memory; none is read on the host.
 *   chars    uint8 [total], the strings one after another;
 *   offsets  int32 [n_strings + 1], ascending, offsets[0] == 0; string j is
 *     chars[offsets[j] .. offsets[j + 1]) and total == offsets[n_strings].  A
 *     string with offsets[j] < 0, offsets[j + 1] < offsets[j] or offsets[j + 1]
 *     > offsets[n_strings] is DROPPED on the device (nothing of chars outside
 *     [0, offsets[n_strings]) is ever read); chars == NULL drops every string;
 *   anchors  int32 [n_strings, 2] (x, y): the top left pixel of the string's
 *     first glyph cell; any int32 value is legal;
 *   scales   uint8 [n_strings], or NULL with `scale` for all strings; 1..4.  A
 *     per-string value outside 1..4 drops that string;
 *   colors   uint8 [n_colors, 3]; n_colors == 1 is one colour for all strings,
 *     otherwise n_colors == n_strings, one row per string;
 *   plate_colors  the same convention; n_plate_colors == 0: no plates.
 * glyphs   character i of a string with scale s and anchor (x, y) has its cell
 *   origin at (x + 6 i s, y), in int64.  Its glyph pixel (column c, row r),
 *   when lit, covers the s x s block whose top left is (x + (6 i + c) s,
 *   y + r s).  The advance is 6 s, the cell height 7 s.  A byte outside
 *   0x20..0x7E draws the glyph of '?'.
 * plate    with plates, a string of n >= 1 characters also owns the rectangle
 *   [x - s, x + (6 n - 1) s + s) x [y - s, y + 7 s + s), shown in its plate
 *   colour.  An empty string draws nothing.
 * stacking on each pixel the string with the LARGEST index wins, by a glyph
 *   pixel or by a plate pixel; within one string a glyph pixel beats a plate
 *   pixel.  A later string's plate therefore covers an earlier string's
 *   glyph, as a later cv2.putText would.  A pixel no string owns keeps its
 *   bytes exactly.
 * clipping pixels off the canvas are skipped.  Only the characters with a
 *   glyph column on the canvas are visited, and the plate is cut to the
 *   canvas first: the work per string is bounded by the canvas, not by its
 *   length.
 * limits   n_strings < 2^30; total < 2^31 (it is an int32).
 * The workspace is one uint32 key per pixel, (string + 1) << 1 | is_glyph,
 * raised with an atomic max; one call clears it, stamps every string and
 * resolves into the image: three launches whatever n_strings is.  Enqueues on
 * `stream`; reads nothing back.  PGNN_E_INVALID (nothing enqueued): width or
 * height outside 1..4096; `scale` outside 1..4 when scales is NULL; n_strings
 * outside 0..2^30-1; n_colors not 1 or n_strings; n_plate_colors not 0, 1 or
 * n_strings; a null colour table with a non-zero count; for n_strings > 0 a
 * null image, offsets, anchors or workspace.  n_strings == 0 returns 0 and
 * enqueues nothing.  PGNN_E_WORKSPACE: workspace_bytes below
 * pgnn_render_text_workspace_bytes (which is 0 for a canvas out of range).  */
size_t pgnn_render_text_workspace_bytes(int32_t width, int32_t height);
int pgnn_render_text(uint8_t *image, int32_t width, int32_t height,
                     const uint8_t *chars, const int32_t *offsets,
                     int64_t n_strings, const int32_t *anchors,
                     const uint8_t *scales, int32_t scale,
                     const uint8_t *colors, int64_t n_colors,
                     const uint8_t *plate_colors, int64_t n_plate_colors,
                     void *workspace, size_t workspace_bytes, void *stream);
int pgnn_render_font(uint8_t *table_host /* [95 * 7] */);

/* ---- PNG scanline unfilter: an inflated 8-bit PNG stream -> pixels ---------
 * The second half of a PNG decode (the first, inflate, stays on the host:
 * pointgnn_amd/png.py).  `raw` is the inflated IDAT stream of a non-interlaced
 * file of bit depth 8 on the device: `height` rows of 1 + width * C bytes, a
 * filter byte (0..4) followed by the filtered bytes.  C follows color_type:
 *   0 grey C = 1, 2 RGB C = 3, 3 palette index C = 1, 4 grey + alpha C = 2,
 *   6 RGBA C = 4.
 * Filter arithmetic (PNG specification, section 9; modulo 256 per byte): with
 * a = the byte C positions to the left, b = the byte above, c = the byte above
 * and C to the left, each 0 outside the image, the reconstructed byte is the
 * filtered byte plus
 *   type 0 (None) 0, 1 (Sub) a, 2 (Up) b, 3 (Average) (a + b) >> 1 with the
 *   sum in at least 9 bits, 4 (Paeth) the Paeth predictor: p = a + b - c,
 *   pa = |p - a|, pb = |p - b|, pc = |p - c|; a if pa <= pb && pa <= pc, else
 *   b if pb <= pc, else c (the order of the tests decides ties).
 * A filter byte above 4 reconstructs like None (png.inflate rejects it first).
 * image uint8 [height, width, 3], channel order R, G, B (bgr = 0) or B, G, R
 * (bgr != 0, cv2.imread's layout):
 *   grey is replicated into the three channels; alpha is dropped, not
 *   composited (cv2.imread's default flag does the same); a palette index i
 *   gives palette[i] (device uint8 [palette_entries, 3] RGB, entries 1..256),
 *   an index >= palette_entries gives (0, 0, 0).
 * One workgroup walks the image in a skewed wavefront (lane = row; bands of
 * rows for taller images, whose last unfiltered row passes through the
 * workspace).  Enqueues on `stream`; reads nothing back.
 * PGNN_E_INVALID (nothing enqueued, pgnn_last_error names the entry): width or
 * height < 1 or a stream size beyond int64, color_type not one of 0, 2, 3, 4,
 * 6, a null pointer, color_type 3 without a palette of 1..256 entries;
 * PGNN_E_WORKSPACE: workspace_bytes below pgnn_png_unfilter_workspace_bytes
 * (which is 0 for sizes out of range).                                       */
size_t pgnn_png_unfilter_workspace_bytes(int64_t width, int64_t height);
int pgnn_png_unfilter(const uint8_t *raw, int64_t width, int64_t height,
                      int32_t color_type, const uint8_t *palette,
                      int32_t palette_entries, int32_t bgr, void *workspace,
                      size_t workspace_bytes, uint8_t *image, void *stream);

/* ---- PNG encode: a device image -> a zlib stream ("pgnn deflate v1") --------
 * The compressed half of writing an 8-bit RGB PNG (the file around it, and the
 * IDAT CRC, stay on the host: pointgnn_amd/png.py).  Only the compressed bytes
 * leave the device.  The output is defined to the bit and is a pure function
 * of (image, chunk_bytes); tests/_deflate_cases.py restates it in Python.
 *
 * input    image: device uint8 [height, width, 3], R, G, B; row y starts at
 *   image + y * row_stride_bytes (row_stride_bytes >= 3 * width; the 3 * width
 *   bytes of a row are contiguous).  height, width >= 1.
 *   S is the PNG scanline stream: every row is one filter byte 0 followed by
 *   its 3 * width bytes.  R = 3 * width + 1 is its row stride, n = height * R
 *   its length.  (What render.png_bytes hands zlib: filter type 0 on every
 *   row.)
 * chunks   C = chunk_bytes, a multiple of 256 with 256 <= C <= 32768.  Chunk c
 *   covers S[c C, min(n, (c + 1) C)); K = ceil(n / C) chunks, compressed
 *   independently of each other.
 * tokens   of a chunk [a, e): parse greedily from i = a.  The candidate
 *   distances, in this order, are D = (1, 3, R); R is dropped when R > 32768.
 *   Candidate d is valid at i only if i - d >= a (a match never reads before
 *   its own chunk).  L_d(i) is the largest L <= min(258, e - i) with
 *   S[i + j] == S[i + j - d] for all j < L (sources may overlap the match, as
 *   in deflate); 0 for a candidate that is not valid.  Take the largest L_d,
 *   ties to the earlier entry of D.  If it is >= 3 emit the match (L, d) and
 *   advance i by L; otherwise emit the literal S[i] and advance i by 1.
 * bits     each chunk is ONE block with the fixed Huffman codes of RFC 1951
 *   3.2.6 (BTYPE = 01): literals 0..143 in 8 bits, 144..255 in 9, length
 *   codes 257..285 with their extra bits (258 is code 285), 5-bit distance
 *   codes with their extra bits, end-of-block = code 256.  BFINAL is 1 on the
 *   last chunk only.  After every chunk but the last comes an empty stored
 *   block: the header bits 000, zero bits to the next byte boundary, the bytes
 *   00 00 FF FF -- so every chunk starts on a byte boundary.  The last chunk
 *   is padded with zero bits to a byte boundary.
 * wrapper  the bytes 78 01, the blocks, the Adler-32 of S, big-endian.  With
 *   (A, B) of a chunk started at (1, 0), two neighbours combine as
 *     A = (A1 + A2 - 1) mod 65521,  B = (B1 + B2 + len2 * (A1 - 1)) mod 65521
 *   and the trailer is B << 16 | A of the whole stream.
 * capacity a chunk of len stream bytes takes at most
 *     slot(len) = floor((9 len + 20) / 8) + 4 bytes
 *   (3 header bits, at most 9 bits per byte -- the dearest match, length 3 at
 *   a distance with 13 extra bits, is 25 bits --, 7 bits of end-of-block, 3
 *   bits of stored header, padding, 4 bytes), so with n = q C + r, 0 <= r < C,
 *     out_capacity = 6 + q slot(C) + (r > 0 ? slot(r) : 0)
 *   bytes always suffice; the entry requires at least that many.
 * out      device uint8 [out_capacity], 4-byte aligned; *out_bytes_dev (device
 *   int64) receives the stream's length, out[0 .. length) the stream; no byte
 *   at or beyond `length` is written.  The length exists on the device only:
 *   nothing is read back here.
 * Three launches on `stream`: one workgroup per chunk, at most one per CU, the
 * rest of the chunks taken in turn (the chunk in LDS, match
 * lengths from 32-byte compare masks, the greedy chain through per-segment
 * exits, bits packed in LDS and stored as whole slots), one workgroup that
 * scans the chunks' byte counts and Adler pairs, one that packs the slots into
 * `out` a dword per lane (csrc/png_encode.hip).
 * PGNN_E_INVALID (nothing enqueued): height or width < 1, a stream length
 * beyond int64 or more than 2^31 - 1 chunks; chunk_bytes not a multiple of 256
 * in 256..32768; row_stride_bytes < 3 * width; a null pointer; `out` not
 * 4-byte or `workspace` not 16-byte aligned; out_capacity below the formula.
 * PGNN_E_WORKSPACE: workspace_bytes below
 * pgnn_png_encode_workspace_bytes (which is 0 for arguments out of range).    */
size_t pgnn_png_encode_workspace_bytes(int64_t height, int64_t width,
                                       int32_t chunk_bytes);
int pgnn_png_encode(const uint8_t *image, int64_t height, int64_t width,
                    int64_t row_stride_bytes, int32_t chunk_bytes,
                    void *workspace, size_t workspace_bytes, uint8_t *out,
                    int64_t out_capacity, int64_t *out_bytes_dev, void *stream);

/* ---- diagnostics (not part of the reference-facing surface) -------------- */
/* Process-wide knobs for benchmarks and tests; see "Conventions".  Keys:
 *   launch shape   scatter_rows_per_wave, scatter_nt, mlp_blocks_per_cu,
 *                  edge_msub, pool_msub, mlp_pool_pct, wgrad_wg_target,
 *                  ws_xcds, ws_prio, ws_pool_pct, ws_chunk, ws_balance, ws_reserve
 *   graph builder  graph_max_wgs (cap on the workgroups of one builder launch;
 *                  every builder kernel strides over its work), graph_lds_pad
 *                  (bytes of dynamic LDS every builder launch asks for without
 *                  using them: such a workgroup cannot be placed beside one of
 *                  the weights-stationary kernels); with ws_reserve they put
 *                  the builder on CUs the fused kernels leave free (measured:
 *                  no net gain; default 0 = off)
 *   kernel choice  b16_force (1: pgnn_edge_mlp_scatter_max_bf16x3_fwd also
 *                  takes lists of a few tiles, where it otherwise answers
 *                  PGNN_E_UNSUPPORTED: the parity tests on small fixtures;
 *                  likewise the f16x2 edge and pooling entries), f16_pool (0:
 *                  pgnn_point_set_pooling_f16x2_fwd declines, i.e. 'f16x2'
 *                  models pool in fp32; 2: it ignores hidden_image: same-box
 *                  A/Bs; default 1),
 *                  mlp_debug bits 2048 / 4096 (edge stage: LDS-tile kernel /
 *                  weights-stationary kernel), 8192 / 16384 (pooling stage),
 *                  1024 (pooling hidden layers through the LDS tile), 32 / 128
 *                  (scatter-max epilogue forms), 512 (4-wave small-row kernel)
 *   ablations      NOT in this library: mlp_debug bits 1 / 2 / 4 (drop gather
 *                  loads / last GEMM / epilogue: wrong results, timing only)
 *                  and graph_debug bit 1 (skip the kd-tree replica) exist only
 *                  in diagnostic builds (-DPGNN_DIAG, tools/build_variant.py);
 *                  the default build rejects them with PGNN_E_INVALID and
 *                  compiles their code out
 * Every key accepted here leaves results bit-identical (tested).
 * Returns 0, or PGNN_E_INVALID for an unknown key / value out of range.     */
int pgnn_set_tunable(const char *key, int value);
/* What the compiler and the occupancy calculator say about one of the 16-row
 * per-vertex kernels: "vertex_pre_edge", "vertex_update_pre_edge",
 * "vertex_mlp2" (host-sized form) or the same with "_dyn" (capacity form,
 * which strides over its tiles and is built for two workgroups per CU).
 * lds_bytes < 0: the dynamic LDS of that kernel's last launch in this process
 * (PGNN_E_INVALID when there was none).  Writes the registers per thread, the
 * scratch bytes per thread, the workgroups of the launch's block size that
 * fit one CU, and the LDS bytes the answer is for.                           */
int pgnn_kernel_occupancy(const char *kernel, int64_t lds_bytes,
                          int32_t *vgprs, int32_t *scratch_bytes,
                          int32_t *workgroups_per_cu, int64_t *lds_used);
/* Device buffer for per-tile cycle stamps of the fused kernels
 * (tools/tile_timeline.py, tools/ws_timeline.py); NULL disables.           */
int pgnn_set_debug_buffer(void *device_ptr);

#ifdef __cplusplus
}
#endif
#endif /* POINTGNN_HIP_H_ */
