/*
 * gpd_hip.h — C-ABI of libgpd_hip.so, the MI355X (gfx950) implementation of the
 * GPD hot path: candidate search -> grasp image -> LeNet score.
 *
 * Everything here is `extern "C"`, plain pointers and sizes.  Host buffers are
 * owned by the caller, device memory is owned by the context.  A context is not
 * thread-safe (the reference's GraspDetector is not either: grasp_detector.cpp:192-328
 * is called from one thread); different contexts — on different devices or on the
 * same one — may be driven from different threads.  The hand / image geometry and
 * the view points live in one constant block per device: contexts on a device
 * that agree on them overlap freely, a context with different values waits for
 * the device before it loads its own (correct, but serialising).
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference tree).  Return value: 0 on success, <0 on error
 * (gpd_hip_last_error() gives the text).  Nothing throws across the boundary.
 */
#ifndef GPD_HIP_H_
#define GPD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_MAX_SLOTS 24 /* num_hand_axes * num_orientations upper bound */

/* Error codes (negative). */
#define GPD_OK 0
#define GPD_ERR_INVALID (-1)   /* bad argument                                   */
#define GPD_ERR_HIP (-2)       /* a HIP runtime call failed                      */
#define GPD_ERR_CAPACITY (-3)  /* a neighbourhood exceeded the LDS list capacity */
#define GPD_ERR_STATE (-4)     /* call order violated (no cloud / no weights)    */

/* How Classifier::classifyImages' dot products are summed (gpd_hip_set_lenet_mode):
 *  GPD_LENET_SPLIT      (default) conv1 on the int8 matrix pipe — exact integer dot products of the u8 inputs with 32-bit
 *                       fixed-point weights, one rounding — conv2 / ip1 on the bf16 matrix pipe with every f32 operand cut
 *                       into three bf16 pieces (six exact piece products per term, f32 accumulation); ip2 as f32 chains.
 *                       The reference's Eigen GEMM fixes no summation order (conv_layer.cpp:54, dense_layer.cpp:11); the
 *                       scores are within 1e-4 of its plain-float path and closer to float64 than an f32 chain's.
 *  GPD_LENET_F32_CHAIN  every dot product as ONE k-ascending f32 fmaf chain on the f32-input MFMA: bit-identical to
 *                       oracle/gpd_oracle.cpp, 1/16 of the matrix rate.  The checker mode. */
#define GPD_LENET_SPLIT 0
#define GPD_LENET_F32_CHAIN 1

/*
 * Parameters of the path.  Field names follow the reference's cfg keys:
 * hand geometry  — cfg/hand_geometry.cfg:8-12, candidate/hand_geometry.cpp:25-30
 * image geometry — cfg/image_geometry_15channels.cfg:8-12, descriptor/image_geometry.cpp:24-28
 * search         — grasp_detector.cpp:67-86 (HandSearch::Parameters)
 * filter         — grasp_detector.cpp:158-174
 */
typedef struct gpd_params {
  double finger_width;        /* 0.01 */
  double hand_outer_diameter; /* 0.12 */
  double hand_depth;          /* 0.06 */
  double hand_height;         /* 0.02 */
  double init_bite;           /* 0.01 */
  double volume_width;        /* 0.10 */
  double volume_depth;        /* 0.06 */
  double volume_height;       /* 0.02 */
  double nn_radius_frames;    /* nn_radius, 0.01 */
  double friction_coeff;      /* 20 */
  double min_aperture;        /* 0.0 */
  double max_aperture;        /* 0.085 */
  double workspace_grasps[6]; /* -1 1 -1 1 -1 1 */
  int32_t image_size;         /* 60 (only 60 is supported, as eigen_classifier.cpp:12) */
  int32_t image_num_channels; /* 1, 3, 12 or 15 (image_strategy.cpp:15-29) */
  int32_t num_orientations;   /* 8 */
  int32_t num_finger_placements; /* 10 */
  int32_t num_hand_axes;      /* 1 */
  int32_t hand_axes[3];       /* {2} */
  int32_t deepen_hand;        /* 1 */
  int32_t min_viable;         /* 6 */
  /* GraspDetector::filterGraspsDirection (grasp_detector.cpp:247-250, 423-456; cfg keys filter_approach_direction,
   * direction, thresh_rad): a valid hand whose approach axis makes an angle acos(direction . approach) > thresh_rad
   * with `direction` is dropped — in the fused entries, on the device, right after the workspace filter. */
  int32_t filter_approach_direction; /* 0 */
  int32_t reserved_;
  double direction[3];        /* 1 0 0 */
  double thresh_rad;          /* 2.0 */
} gpd_params;

/*
 * One grasp candidate = candidate::Hand (include/gpd/candidate/hand.h:80-277,
 * candidate/hand.cpp:24-45) flattened to POD.  `frame` is row-major; its columns
 * are approach | binormal | axis (hand.h getApproach/getBinormal/getAxis).
 */
typedef struct gpd_hand {
  double sample[3];
  double frame[9];
  double position[3];
  double top, bottom, center; /* closing box, hand.h BoundingBox */
  double grasp_width;
  float score;
  int32_t finger_placement_index; /* -1 when no feasible placement exists */
  int32_t set_index;              /* hand set = sample that produced it     */
  int32_t slot;                   /* axis_i * num_orientations + angle_i    */
  uint8_t valid;                  /* HandSet::is_valid_                     */
  uint8_t half_antipodal, full_antipodal;
  uint8_t pad_[5];
} gpd_hand;

typedef struct gpd_hip_ctx gpd_hip_ctx;

/* Fill `p` with the defaults of cfg/eigen_params.cfg + cfg/hand_geometry.cfg +
 * cfg/image_geometry_15channels.cfg. */
void gpd_hip_default_params(gpd_params *p);

/* Create a context on HIP device `device`.  Replaces the constructor work of
 * GraspDetector (grasp_detector.cpp:5-190) that sizes the path. */
int gpd_hip_create(int device, const gpd_params *params, gpd_hip_ctx **out);
void gpd_hip_destroy(gpd_hip_ctx *ctx);
const char *gpd_hip_last_error(void);

/* LeNet parameters, raw float32 exactly as the files read by
 * EigenClassifier::EigenClassifier (net/eigen_classifier.cpp:28-50):
 * conv1 [20][C*25] row-major, conv2 [50][500] row-major, ip1 column-major
 * 500 x 7200 over the pixel-major flatten (eigen_classifier.cpp:103-107,
 * dense_layer.cpp:7), ip2 column-major 2 x 500.  Copied to the device once.
 * All conv1 / conv2 / ip1 weights must be finite (GPD_ERR_INVALID otherwise): the f32 chain's conv1 skips input
 * patches that are all zero, which is exact for finite weights only (0 * inf = NaN), and the split
 * path's fixed-point / bf16 pieces are defined for finite numbers. */
int gpd_hip_set_lenet_weights(gpd_hip_ctx *ctx, int channels,
                              const float *conv1_w, const float *conv1_b,
                              const float *conv2_w, const float *conv2_b,
                              const float *ip1_w, const float *ip1_b,
                              const float *ip2_w, const float *ip2_b);

/* GPD_LENET_SPLIT or GPD_LENET_F32_CHAIN (above) for every later scoring call of the context. */
int gpd_hip_set_lenet_mode(gpd_hip_ctx *ctx, int mode);

/* The network of the reference's PyTorch scripts (pytorch/network.py::Net, trained by pytorch/train_net3.py) applies a
 * ReLU after conv1 and after conv2; EigenClassifier, the Caffe prototxts and the shipped OpenVINO IR have none.  on = 1:
 * every later scoring call of the context (gpd_hip_score, gpd_hip_detect*, gpd_hip_detect_batch[_multi], gpd_hip_replay;
 * gpd_hip_detect_sharded reads each context's own flag) clamps the pooled values of both convolutions at zero — ReLU and a
 * 2x2 max-pool commute — in either scoring mode; on = 0 (default): the reference's Eigen network.  Anything else is
 * GPD_ERR_INVALID.  Context state like the mode: legal before or after the weights, and gpd_hip_set_lenet_weights does not
 * reset it.  gpd_hip_lenet_debug(which = 0 / 1) returns the tensors after the ReLU when it is on. */
int gpd_hip_set_lenet_conv_relu(gpd_hip_ctx *ctx, int on);

/* Net's tensors (a state_dict of pytorch/train_net3.py) -> the layouts gpd_hip_set_lenet_weights takes.  Host only, no
 * context.  conv1_weight [20][C][5][5], fc1_weight [500][7200] over the channel-major flatten (k = channel * 144 + pixel),
 * fc2_weight [2][500], all row-major as torch stores them.
 *   conv1_w_out [20][C*25]  = (float)((double)w * input_scale): the scale the training data was fed with (hdf5_dataset.py:17:
 *                             1/256; exact for a power of two) folded into the weights, so that raw 0..255 images score the same
 *   ip1_w_out   [7200][500] : ip1[(p * 50 + c) * 500 + u] = fc1[u][c * 144 + p]
 *   ip2_w_out   [500][2]    : ip2[j * 2 + u] = fc2[u][j]
 * conv2.weight ([50][20][5][5] = the reference's [50][500]) and the four biases pass through unchanged: hand them to
 * gpd_hip_set_lenet_weights as they are.  Together with gpd_hip_set_lenet_conv_relu(ctx, 1) the context computes Net.
 * GPD_ERR_INVALID: a null pointer, channels not in {1, 3, 12, 15}, a non-finite or non-positive input_scale. */
int gpd_hip_lenet_from_torch(int channels, double input_scale, const float *conv1_weight, const float *fc1_weight,
                             const float *fc2_weight, float *conv1_w_out, float *ip1_w_out, float *ip2_w_out);

/* ---- the shape-general scoring route -------------------------------------------------------------------------------
 * The family of networks the reference's pytorch/network.py describes (its CHANNELS lists; Net and NetCCFFF) on 60x60
 * images:
 *   conv1  channels -> conv1_out, 5x5, valid;  2x2 max-pool;  ReLU when gpd_hip_set_lenet_conv_relu is on
 *   conv2  conv1_out -> conv2_out, 5x5, valid; 2x2 max-pool;  ReLU when gpd_hip_set_lenet_conv_relu is on
 *   fc1    conv2_out * 144 -> fc1_out, ReLU
 *   fc2    fc1_out -> fc2_out, ReLU           only when fc2_out > 0 (NetCCFFF)
 *   last   -> 2 logits;  score = logit1 - logit0
 * Limits (gpd_hip_lenet_shape_check is their one statement): channels in {1, 3, 12, 15}, 1 <= conv1_out <= 64,
 * 1 <= conv2_out <= 128, 1 <= fc1_out <= 1024, 0 <= fc2_out <= 1024.
 * Arithmetic: every multiply-add layer is one f32 chain per output — acc = 0, acc = fmaf(w, x, acc) with k ascending, then
 * acc + bias — with k = (input channel, kh, kw) in the convolutions, k = pixel * conv2_out + channel in fc1 (the project's
 * pixel-major flatten) and k = the hidden index in fc2 and the last layer.  No split-K, no atomics: a score does not depend on
 * the batch it is computed in.  The kernels run the chains on the f32-input matrix instructions of gfx950, which are bit for
 * bit such chains.  The stock shape (C, 20, 50, 500, 0) is legal here; gpd_hip_set_lenet_weights serves it with tuned kernels. */
typedef struct gpd_lenet_shape {
  int32_t channels, conv1_out, conv2_out, fc1_out, fc2_out;
} gpd_lenet_shape;

/* GPD_OK when the shape is within the limits above, GPD_ERR_INVALID (and an error text) otherwise or for a null pointer.  Host only. */
int gpd_hip_lenet_shape_check(const gpd_lenet_shape *shape);

/* A state dict of pytorch/network.py::Net / NetCCFFF -> the layouts gpd_hip_set_lenet_net takes.  Host only, no context.
 * torch_tensors, row-major as torch stores them (F1 = conv1_out, F2 = conv2_out, H1 = fc1_out, H2 = fc2_out):
 *   [0] conv1.weight [F1][C][5][5]   [1] conv1.bias [F1]   [2] conv2.weight [F2][F1][5][5]   [3] conv2.bias [F2]
 *   [4] fc1.weight [H1][F2*144] over the channel-major flatten (k = channel * 144 + pixel)     [5] fc1.bias [H1]
 *   H2 > 0:  [6] fc2.weight [H2][H1]  [7] fc2.bias [H2]  [8] fc3.weight [2][H2]  [9] fc3.bias [2]
 *   H2 == 0: [6] fc2.weight [2][H1]   [7] fc2.bias [2]   [8], [9] unused (may be null)
 * out, caller-allocated with the same element counts (the route's layouts):
 *   [0] [F1][C*25] = (float)((double)w * input_scale)      [2] [F2][F1*25] unchanged      biases [1] [3] [5] [7] [9] unchanged
 *   [4] [F2*144][H1]: out[(p * F2 + c) * H1 + u] = fc1[u][c * 144 + p]
 *   [6] [H1][N]:      out[j * N + u] = fc2[u][j], N = H2 (or 2 when H2 == 0)
 *   [8] [H2][2]:      out[j * 2 + u] = fc3[u][j]           (H2 > 0 only)
 * GPD_ERR_INVALID: a null pointer among the used ones, a shape outside the limits, a non-finite or non-positive input_scale. */
int gpd_hip_lenet_net_from_torch(const gpd_lenet_shape *shape, double input_scale, const float *const torch_tensors[10],
                                 float *const out[10]);

/* Installs a network of `shape` (tensors in the layouts gpd_hip_lenet_net_from_torch writes).  Every later scoring call of
 * the context — gpd_hip_score, gpd_hip_detect*, gpd_hip_detect_batch[_multi], gpd_hip_detect_sharded (each context its own),
 * gpd_hip_detect_sis, gpd_hip_score_given, gpd_hip_replay — takes the general route, until gpd_hip_set_lenet_weights
 * returns the context to the stock one.  gpd_hip_set_lenet_conv_relu is honoured as on the stock route;
 * gpd_hip_set_lenet_mode is accepted and IGNORED: this route computes the chain by default; gpd_hip_set_lenet_net_mode
 * (below) chooses its other arithmetic.  shape->channels must equal the
 * context's image_num_channels; every weight and bias must be finite (subnormal ones are kept and computed with: the
 * route does not flush); the LDS the shape needs is checked here, not at launch (GPD_ERR_INVALID each).
 * Order: install, THEN gpd_hip_reserve.  The route's scratch depends on the shape, so an install frees the scratch of every
 * lane; a reservation made before it is void for the scoring buffers, which then grow (booked) in the first pass of each lane. */
int gpd_hip_set_lenet_net(gpd_hip_ctx *ctx, const gpd_lenet_shape *shape, const float *const tensors[10]);

/* The arithmetic of the general route, per context:
 *  GPD_LENET_NET_CHAIN  (default) the f32 chains above, bit for bit the CPU checker's.
 *  GPD_LENET_NET_SPLIT  v_mfma_f32_16x16x32_bf16 (16 times the matrix rate of the f32-input instruction) on exactly split
 *                       operands, f32 accumulation:
 *    pieces   a = h + m + l with h = bf16(a), m = bf16(a - h), l = bf16(a - h - m), round to nearest even, the residuals
 *             exact in f32 (gpd_hip_bf16_split3 is the definition); the sum is exact for an f32 whose pieces stay normal.
 *    conv1    the u8 inputs are ONE exact piece (255 has 8 significant bits), the weights (input scale folded in) three:
 *             three exact products per term, nothing dropped.
 *    conv2, fc1, fc2   both operands three pieces; the six products h*h, h*m, m*h, h*l, l*h, m*m accumulate in f32; m*l, l*m
 *             and l*l are dropped (below 2^-24 of the term).  Then, as in the chain: the max over the 2x2 window on the
 *             accumulators, + bias, the optional ReLU.
 *    last     the two logits stay the chain's two fmaf chains: given the last hidden tensor they are the chain bit for bit.
 *    order    no split-K, no atomics; which k a step of 32 holds and the order of the products inside it are fixed by the
 *             shape alone (convolutions: chunks of 8 input channels, inside a chunk k = tap * 8 + channel; fc1: k = pixel *
 *             round_up(conv2_out, 8) + channel; fc2: the hidden index).  A score depends neither on the batch an image is in
 *             nor on its position nor on the chunk, and two runs give the same bits.
 *    domain   bf16 has f32's exponent range (scalings such as 2^+-100 are fine).  The accuracy statement covers operands that
 *             are zero or at least 2^-100 in magnitude: below 2^-110 the lower pieces fall into bf16's subnormal range, where
 *             the matrix pipe's behaviour is unmeasured.  Smaller operands are computed with unspecified accuracy and are NOT
 *             refused (activations cannot be policed).
 *  Context state like gpd_hip_set_lenet_conv_relu: legal before or after gpd_hip_set_lenet_net; neither an install nor
 *  gpd_hip_set_lenet_weights resets it.  The weight piece tables are built when network and mode meet, whichever call comes
 *  second (the LDS of the split kernels is checked there too), and freed with the network.  The two modes' scratch differs, so
 *  a mode change with a network installed frees the general-route scratch of every lane, as an install does: install, set the
 *  mode, THEN gpd_hip_reserve.  gpd_hip_reserve and gpd_hip_lenet_net_info price the mode in force; the mode never falls back.
 *  Any other value, or a null context: GPD_ERR_INVALID, "gpd_hip_set_lenet_net_mode: bad argument". */
#define GPD_LENET_NET_CHAIN 0
#define GPD_LENET_NET_SPLIT 1
int gpd_hip_set_lenet_net_mode(gpd_hip_ctx *ctx, int mode);

/* The three bf16 pieces (bit patterns) of n floats, as the split kernels and their weight tables make them.  Host only, no
 * context.  GPD_ERR_INVALID: n < 0, or a null pointer with n > 0. */
int gpd_hip_bf16_split3(const float *x, long long n, uint16_t *h, uint16_t *m, uint16_t *l);

/* Activations of the last scoring call that took the general route (lane 0; n images, at most the first chunk), plain
 * row-major f32: which = 0: pool1 [n][F1][28][28], 1: pool2 [n][F2][12][12], 2: fc1 [n][H1], 3: fc2 [n][H2] (H2 > 0 only),
 * 4: logits [n][2] — pool tensors after the ReLU when it is on.  In GPD_LENET_NET_SPLIT a tensor the device holds as bf16
 * pieces is returned as the exact sum of its pieces.  GPD_ERR_INVALID when the last scoring call did not take
 * the general route (how a caller learns which route ran). */
int gpd_hip_lenet_net_debug(gpd_hip_ctx *ctx, int which, int n, float *out);

/* info[0] images per chunk, [1] scratch bytes per image, [2] the largest static + dynamic LDS of the route's kernels
 * (bytes) — each of the mode in force — [3] multiply-adds per image (the algorithmic count, either mode).  GPD_ERR_STATE without an installed network. */
int gpd_hip_lenet_net_info(gpd_hip_ctx *ctx, long long info[4]);

/* Replaces Classifier::classifyImages (net/classifier.h:70-71,
 * eigen_classifier.cpp:59-79).  images: n contiguous 60x60xC u8 HWC images
 * (cv::Mat CV_8UC(C) layout); scores[i] = logit1 - logit0.
 * images == NULL scores the images left on the device by gpd_hip_images. */
int gpd_hip_score(gpd_hip_ctx *ctx, const uint8_t *images, int n, float *scores);

/* Upload the processed cloud: what HandSearch::searchHands and
 * ImageGenerator::createImages read from util::Cloud (hand_search.cpp:28-31,
 * 160-165; image_generator.cpp:24-29): float32 xyz (AoS), float32 normals
 * (AoS), camera source n_cams x P (row per camera, 0/1), view points 3 doubles
 * per camera.  1 <= num_cams <= 32 (GPD_ERR_INVALID beyond: the kernels carry the
 * cameras that see a neighbourhood as a 32-bit mask). */
int gpd_hip_upload_cloud(gpd_hip_ctx *ctx, const float *xyz, const float *normals,
                         int num_points, const int32_t *cam_source, int num_cams,
                         const double *view_points);

/* SURVEY §8f rank 3, the step after selectGrasps: replaces Clustering::findClusters (clustering.cpp:5-105).
 * hands: n records (axis = third column of `frame`, `position`); scores: their scores as doubles (Hand keeps a double,
 * hand.h:253; the record's float is not read).  A seed hand with at least min_inliers inliers (axis within 12 degrees,
 * position within 0.05 m and within 0.005 m of the seed's axis line, clustering.cpp:9-13) yields a cluster: the seed's
 * record with position = mean inlier position, out_scores = lower bound of the 99 % confidence interval of the inlier
 * scores (the record's float score is its rounding), out_src = index of the seed; clusters come in seed order.
 * remove_inliers != 0: a hand that was an inlier of an earlier seed is skipped by the later ones (:36, :70-72).
 * out / out_scores / out_src must hold n entries. */
int gpd_hip_find_clusters(gpd_hip_ctx *ctx, const gpd_hand *hands, const double *scores, int n, int min_inliers, int remove_inliers,
                          gpd_hand *out, double *out_scores, int32_t *out_src, int *num_out);

/* SURVEY §8f rank 2 (the step before the normals): replaces the point-cloud part of Cloud::filterWorkspace
 * (util/cloud.cpp:243-266) followed by Cloud::voxelizeCloud (util/cloud.cpp:286-348) as
 * CandidatesGenerator::preprocessPointCloud runs them on a cloud without normals (candidates_generator.cpp:19-26).
 * xyz: num_points x 3 float32 without NaN/Inf (pcl::removeNaNFromPointCloud ran at load time, cloud.cpp:154-164);
 * cam_source: num_cams rows of num_points (may be NULL with num_cams = 0).
 * workspace: 6 doubles (min/max x, y, z; strict comparisons) or NULL = no cut.  voxel_size <= 0: no voxeliser, the
 * points inside the workspace come back in input order with their camera-source columns.  voxel_size > 0: the points
 * the reference's std::set keeps under its "differs" comparator (cloud.h:105-122) — not one per voxel, see
 * gpd_amd/csrc/preprocess.hip — replaced by their voxel corner min + voxel_size * index, in the set's iteration order,
 * camera source reduced to (== 1 ? 1 : 0) as cloud.cpp:325-327.
 * xyz_out / cam_out (num_cams rows of *num_out) / src_out (input index per output point, may be NULL) must hold
 * num_points entries.  kernel_ms (may be NULL) receives the device time of the kernels.  The context's uploaded cloud
 * is not touched: gpd_hip_upload_cloud + gpd_hip_estimate_normals follow with the result. */
int gpd_hip_preprocess_cloud(gpd_hip_ctx *ctx, const float *xyz, const int32_t *cam_source, int num_points, int num_cams,
                             const double *workspace, float voxel_size, float *xyz_out, int32_t *cam_out, int32_t *src_out,
                             int *num_out, float *kernel_ms);

/* SURVEY §8f rank 1 (the step that feeds the path its normals): replaces Cloud::calculateNormals
 * (util/cloud.cpp:451-476) = calculateNormalsOMP (:497-535, radius search, PCA, flip towards the
 * view point) + reverseNormals (:573-604), on the cloud uploaded last (its normals argument may
 * be zeros).  normals receives num_points*3 floats and also replaces the device copy. */
int gpd_hip_estimate_normals(gpd_hip_ctx *ctx, double radius, float *normals);

/* Replaces Cloud::sampleAbovePlane (util/cloud.cpp:407-436; CandidatesGenerator::preprocessPointCloud calls it between
 * the normals and subsample, candidates_generator.cpp:32-34): PCL 1.9's SACSegmentation with SACMODEL_PLANE, SAC_RANSAC,
 * setDistanceThreshold(threshold) and setOptimizeCoefficients(optimize), then ExtractIndices(negative) — the definition
 * is DESIGN §7.  The reference's values: threshold 0.01, max_iterations 50, probability 0.99, optimize 1.
 * On the cloud uploaded last (its normals are not read).  indices_out must hold num_points entries: the points farther
 * than the threshold from the final plane, ascending, *num_out of them.  *num_out = 0 is the reference's "plane fit
 * failed" (no model, or every point on the plane): the caller keeps its sample indices then.  coeffs: the final plane
 * (a, b, c, d), zero without a model; *num_inliers: points within the threshold of it; *iterations: the hypotheses RANSAC
 * evaluated.  Capacities (GPD_ERR_CAPACITY beyond them): max_iterations <= 1023, and the draws of one call may touch at
 * most 7680 positions of PCL's shuffled index list (3 per try: only clouds with many degenerate draws come near it). */
int gpd_hip_sample_above_plane(gpd_hip_ctx *ctx, double threshold, int max_iterations, double probability, int optimize,
                               int32_t *indices_out, int *num_out, float coeffs[4], int *num_inliers, int *iterations);

/* Replaces Cloud::refineNormals(k) (util/cloud.cpp:176-204; CandidatesGenerator::preprocessPointCloud calls it after the
 * normals when cfg refine_normals_k > 0, candidates_generator.cpp:28-30): pcl::search::KdTree::nearestKSearch of every
 * point (itself included, FLANN's float d2, ascending by (d2, index), k clamped to the cloud's size), then
 * pcl::NormalRefinement — the definition is DESIGN §7.  The reference's values: max_iterations 15, convergence_threshold
 * 1e-5; threshold 0 runs exactly max_iterations passes.  On the normals of the cloud uploaded last, or last estimated
 * (gpd_hip_estimate_normals); the result replaces the device copy, so a following gpd_hip_detect uses it without an upload.
 * normals_out receives num_points*3 floats (NaN: a singularity, as in the reference); *iterations_out: the passes run;
 * ddot_out (may be NULL, else max_iterations floats): the mean dot product of every pass, the value the stop rule tests;
 * *num_nan_out: normals with a non-finite component; kernel_ms (may be NULL): the kNN kernel, the refinement passes launched
 * (one past a stop is launched speculatively), the whole call, in ms.  GPD_ERR_INVALID: a NULL argument, k < 1,
 * max_iterations < 0, a negative or non-finite threshold, or no cloud.  Capacity (GPD_ERR_CAPACITY beyond it): k <= 256. */
int gpd_hip_refine_normals(gpd_hip_ctx *ctx, int k, int max_iterations, float convergence_threshold, float *normals_out, int *iterations_out,
                           float *ddot_out, int *num_nan_out, float kernel_ms[3]);

/* Replaces Cloud::removeStatisticalOutliers (util/cloud.cpp:166-174, which the reference declares and never calls):
 * pcl::StatisticalOutlierRemoval with setMeanK(mean_k) and setStddevMulThresh(stddev_mult) — the reference's values are 50
 * and 1.0; the definition is DESIGN §7.  Every point's mean distance to its mean_k nearest neighbours (FLANN's float d2,
 * correctly rounded float sqrt, summed in double in rank order), the mean and standard deviation of those over the cloud
 * (two sequential double sums in index order), and a point is removed iff (double)dist > mean + stddev_mult * stddev; a NaN
 * threshold (equal distances whose variance rounding made negative) removes nothing.
 * Acts on the cloud uploaded last and REPLACES it on the device with the kept points in input order: their normals and
 * camera-source rows follow them (unlike the reference's sor.filter(*cloud_processed_), which leaves both misaligned), the
 * grid is rebuilt, and a following gpd_hip_estimate_normals / gpd_hip_detect uses the kept cloud without an upload — sample
 * indices then count in the kept cloud.  kept_out (room for num_points entries): the kept input indices, ascending, *num_kept
 * of them; stats: mean, stddev, threshold; dist_out (may be NULL, else num_points floats): the mean distances; kernel_ms (may be
 * NULL): the distance kernel, the compaction, the whole call, in ms.
 * GPD_ERR_INVALID (the cloud stays as it was): a NULL argument, mean_k < 1, a non-finite stddev_mult, no cloud, fewer than
 * mean_k + 1 points (PCL reads past the lists its search returned there), or a threshold below every distance (no point would
 * be left).  Capacity (GPD_ERR_CAPACITY beyond it): mean_k <= 255. */
int gpd_hip_remove_statistical_outliers(gpd_hip_ctx *ctx, int mean_k, double stddev_mult, int32_t *kept_out, int *num_kept, double stats[3],
                                        float *dist_out, float kernel_ms[3]);

/* Replaces CandidatesGenerator::generateGraspCandidateSets ->
 * HandSearch::searchHands (candidates_generator.cpp:62-69, hand_search.cpp:24-64)
 * for samples given by index (Cloud::getSampleIndices).  Writes
 * num_sets * num_slots hands (set-major, slot-minor; num_slots = num_hand_axes *
 * num_orientations); samples without a frame neighbourhood are dropped before
 * sets are numbered (frame_estimator.cpp:24-29).  hands must hold
 * num_samples * num_slots records. */
int gpd_hip_search(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples,
                   gpd_hand *hands, int *num_sets);

/* The same for samples given by coordinates (Cloud::getSamples; hand_search.cpp:37-39,
 * FrameEstimator::calculateLocalFrames(cloud, samples, ...) frame_estimator.cpp:38-65):
 * samples_xyz holds 3 doubles per sample.  As in the reference the kd-tree queries use the float
 * cast of the sample (eigenVectorToPcl) while the hand frame keeps the double. */
int gpd_hip_search_samples(gpd_hip_ctx *ctx, const double *samples_xyz, int num_samples,
                           gpd_hand *hands, int *num_sets);

/* replaces HandSearch::reevaluateHypotheses (hand_search.cpp:66-134, 190-228;
 * GraspDetector::evalGroundTruth, grasp_detector.cpp:522-526) on the cloud uploaded last (the
 * ground-truth cloud): each hand is checked again with its own frame, `top` and
 * finger_placement_index; labels[i] = 1 for a full antipodal grasp, half_antipodal /
 * full_antipodal of the records are rewritten.  Reuses the search buffers: hands of an earlier
 * gpd_hip_search can no longer be passed to gpd_hip_images afterwards. */
int gpd_hip_reevaluate(gpd_hip_ctx *ctx, gpd_hand *hands, int num_hands, int32_t *labels);

/* The ground-truth cloud of DataGenerator (data_generator.cpp:98-131: the object's mesh) as a SECOND cloud slot of the
 * context, with its own grid and search scratch: xyz / normals as gpd_hip_upload_cloud takes them, no cameras
 * (reevaluateHypotheses reads none).  It stays until it is replaced, or cleared with num_points == 0 (the pointers are not
 * read then); gpd_hip_upload_cloud and the detect, batch, reevaluate, normals and preprocess entries do not touch it.
 * Read by gpd_hip_label_view only. */
int gpd_hip_upload_ground_truth(gpd_hip_ctx *ctx, const float *xyz, const float *normals, int num_points);

/* BalanceInstances of DataGenerator (data_generator.cpp:406-430) + the order addInstances writes (:432-458) over the labels
 * of a view's n accumulated candidates — host only, no context; the definition gpd_hip_label_view's device selection equals
 * (gpd_amd/csrc/balance_model.h).  With P labels != 0 and N labels == 0: end = min(min(P, N), max_grasps_per_view / 2); out_index
 * receives the first `end` positives, then the first `end` negatives, each in accumulated order; *num_out = 2 * end,
 * *num_positives_out = end.  out_index holds 2 * floor(max_grasps_per_view / 2) entries (or n, if that is less).
 * GPD_ERR_INVALID: n < 0, a NULL labels with n > 0, a NULL count pointer, or a NULL out_index when something is kept. */
int gpd_hip_balance_view(const uint8_t *labels, int n, int max_grasps_per_view, int32_t *out_index, int *num_out, int *num_positives_out);

/* The orders in which DataGenerator stores its shuffled instance sets (data_generator.cpp:219-220) — host only, no context.
 * The reference's std::random_shuffle draws from rand(); here a Fisher-Yates from the back (entry i with entry next() % (i + 1))
 * on the seeded xorshift64 stream described at gpd_detect_job::num_draws, ONE stream from `seed` that runs on through the
 * num_sets sets of sizes[] in order (per object: the training set, then the test set).  out receives the orders back to back
 * (sum of sizes entries): out[k] of a set = the instance that ends up at position k.  GPD_ERR_INVALID: a negative size or a
 * NULL argument. */
int gpd_hip_shuffle_orders(uint32_t seed, const int32_t *sizes, int num_sets, int32_t *out);

/* One view of DataGenerator::generateData (data_generator.cpp:140-213): rounds of createGraspImages (grasp_detector.cpp:458-521)
 * + evalGroundTruth (:522-526) on the cloud uploaded last, against the ground truth of gpd_hip_upload_ground_truth, until
 * min_positives positives have accumulated; then balanceInstances.  Everything stays on the device between the upload of the
 * sample indices and ONE copy of the kept instances: per round only the 56-byte plan summary and 8 bytes of counts come back.
 *  - round r (while positives < min_positives and r < max_rounds; min_positives <= 0: no round) runs what gpd_hip_detect builds
 *    before the LeNet on sample_indices[r * samples_per_round ...] — index search, filterGraspsWorkspace, the direction filter
 *    when set, one image per valid hand, set-major / slot-minor; each round's shadow stream starts at 0; no weights are needed.
 *    The reference's loop has no bound on r and never ends on a view without positives: max_rounds is ours.
 *  - its candidates are checked by reevaluateHypotheses against the ground truth: one neighbourhood list per hand SET with a
 *    candidate (the hands of a set share their sample), labels and flags byte for byte those of gpd_hip_reevaluate.
 *  - images, records and labels are appended to the view's accumulator; EVERY round's indices are shifted by the accumulated
 *    count (the reference shifts only when earlier rounds found positives, :171-180, and then moves the wrong images).
 *  - the kept instances are those of gpd_hip_balance_view over the accumulated labels, positives first.
 * hands[i] is the record gpd_hip_detect_select(num_selected = 0) returns for its round, with score = 0 and the flags of the
 * ground-truth check; labels[i] == hands[i].full_antipodal; src_index[i]: its index in the accumulated candidate list.
 * GPD_ERR_INVALID (before any work): a capacity below 2 * floor(max_grasps_per_view / 2), a sample index out of range.
 * GPD_ERR_STATE: no view cloud or no ground truth.  GPD_ERR_CAPACITY: an accumulator beyond 16 GB. */
typedef struct gpd_label_view_job {          /* zero it first */
  const int32_t *sample_indices;             /* in: max_rounds x samples_per_round, round-major, into the cloud uploaded last */
  int32_t samples_per_round, max_rounds;
  int32_t min_positives;                     /* cfg min_grasps_per_view */
  int32_t max_grasps_per_view;
  uint8_t *images;                           /* out: capacity x 60*60*C, HWC */
  uint8_t *labels;                           /* out: capacity */
  gpd_hand *hands;                           /* out: capacity records (may be NULL) */
  int32_t *src_index;                        /* out: capacity, index into the view's accumulated candidate list (may be NULL) */
  int32_t capacity;                          /* >= 2 * floor(max_grasps_per_view / 2), else GPD_ERR_INVALID before any work */
  uint8_t *all_labels; int32_t all_labels_capacity;  /* out, may be NULL: the label of EVERY accumulated candidate (1 byte each);
                                                        the first all_labels_capacity of them when there are more */
  int32_t *round_counts;                     /* out, may be NULL: max_rounds x {candidates, positives} */
  int32_t rounds_run, num_candidates, num_positives, num_out, num_positives_out;  /* out */
  int32_t gt_neighbourhoods;                 /* out: ground-truth neighbourhood lists built */
  int64_t d2h_bytes;                         /* out: bytes this call copied device -> host */
  float stage_ms[4];                         /* out: search, images, labels, select + gather (HIP events) */
} gpd_label_view_job;
int gpd_hip_label_view(gpd_hip_ctx *ctx, gpd_label_view_job *job);
int gpd_hip_sizeof_label_view_job(void);

/* What the image stage derives from a geometry before it launches a kernel — host only, no context; the definition
 * (gpd_amd/csrc/image_model.h) images_reserve / images_run use.
 *  - window_class: which voxel windows the shadow kernels take for the image volume: 0 the default (a 46^3 window per candidate,
 *    a region of 86^3 voxels per hand set), 1 the wide ones (64^3 / 128^3), 2 the general kernel with a region of the size the
 *    geometry needs; set_sd / set_sr: edge and radius of that region in voxels of 3 mm.
 *  - num_shadow = floor(shadow_length / 0.003) draws per point of a hand set, shadow_length = max(volume_depth,
 *    volume_height / 2, volume_width) (image_15_channels_strategy.h:70-75); (stride_a, stride_c): the
 *    affine map s -> stride_a * s + stride_c (mod 2^32) of 1024 * num_shadow steps of HandSet::fastrand (hand_set.cpp:263-266).
 *  - thr[a][k], a = depth, width, 2 * height: the smallest double x with floor((x / len_a) / (1.0 / 60)) >= k, the cell
 *    formula of image_strategy.cpp:92-102 in its own IEEE operations; thr[a][0] = 0, thr[a][60] = DBL_MAX.
 *  - true_div: 1 when the kernels' division by len_a through RN(1 / len_a) and two FMAs was seen to differ from the IEEE
 *    quotient for one of the extents (they divide for real then).
 * GPD_ERR_INVALID: a NULL argument.  GPD_ERR_CAPACITY: an image volume whose shadow region would exceed 1280^3 voxels. */
typedef struct gpd_image_model {
  int32_t window_class, set_sd, set_sr, num_shadow;
  uint32_t stride_a, stride_c;
  int32_t true_div, reserved_;
  double thr[3][61];
} gpd_image_model;
int gpd_hip_image_model(const gpd_params *params, gpd_image_model *out);
/* ... with the windows of a shadow-jitter setting (gpd_hip_set_shadow_jitter below; 0 or 1, anything else GPD_ERR_INVALID).
 * gpd_hip_image_model is the case 0.  With 1 a candidate's window holds every voxel whose moved point can lie in its box and a
 * set's region likewise — two more voxels on each side of the window, two more of reach — so the stock geometry takes the wide
 * windows (window_class 1) and a wide geometry may take the general kernel; thresholds, num_shadow and the LCG stride do not
 * depend on the setting. */
int gpd_hip_image_model_jitter(const gpd_params *params, int shadow_jitter, gpd_image_model *out);

/* ---- shadow points off the lattice: an opt-in, seeded, per-voxel jitter -------------------------------------------------
 * HandSet::shadowVoxelsToPoints (hand_set.cpp:187-204) moves every shadow voxel's point by ONE N(0,1) draw times 0.3 voxels,
 * the same draw on all three coordinates, from a generator seeded by std::random_device: no two runs of the reference draw
 * alike.  By default this library puts the points on the 3 mm lattice (zero jitter, the policy its oracle is built with).
 * The mode below has the reference's magnitude and arithmetic with a draw that is a pure function of (seed, voxel) — so it
 * does not depend on how a cloud is batched, sharded or resumed.  It is NOT the reference's own, unreproducible stream.
 *
 * The definition (gpd_amd/csrc/jitter_model.h), all integer arithmetic and exact double operations.  mix(z), on 64-bit words:
 *   z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *   return z ^ (z >> 31).
 * Voxel (x, y, z), int32 read as uint32 and zero-extended:  k0 = mix(seed ^ (x | y << 32)), k1 = mix(k0 ^ z), k2 = mix(k1),
 * k3 = mix(k2);  S = the sum of the twelve 16-bit fields of k1, k2, k3;  g = (double)(S - 393210) * (1.0 / 65536.0): Irwin-Hall
 * with twelve terms, mean 0, variance 1 - 2^-32, |g| < 6.  The voxel's point, unfused and in the reference's operand order:
 *   p_a = (double)v_a * 0.003 + (g * 0.003) * 0.3,  a = 0, 1, 2  (|shift| < 5.4 mm per world axis).
 * The box test, the cell lookup and the depth that enters a pixel's mean take the moved point; the order in which points enter
 * a pixel's mean stays lexicographic in the VOXEL; the voxel sets and their intersection over cameras stay on voxels.
 *
 * gpd_hip_set_shadow_jitter: context state like gpd_hip_set_lenet_conv_relu.  on = 0 (default) or 1, anything else is
 * GPD_ERR_INVALID and changes nothing; GPD_ERR_STATE while gpd_hip_detect_batch drives the lanes.  It holds for every later
 * call of the context that makes images: gpd_hip_images, _images_given, _score_given, _detect, _detect_select,
 * _detect_samples, _detect_batch, _detect_batch_multi, _detect_sis, _label_view, _train_append_view, _replay (a resident
 * candidate list is re-launched under the setting in force) and _detect_sharded, where each context applies its OWN setting:
 * the caller sets them alike.  With 1, 3 or 12 channels there is no shadow channel: accepted, changes nothing.  The call waits
 * for the context's streams.  It may change the window class (above), so buffers sized before it can grow at the next call;
 * gpd_hip_reserve after the switch sizes for the setting in force.  The shadow draws a hand set consumes (lcg_draws) do not
 * depend on it. */
int gpd_hip_set_shadow_jitter(gpd_hip_ctx *ctx, int on, uint64_t seed);
/* g of the definition above for n voxels [n][3].  Host only, no context.  GPD_ERR_INVALID: a NULL pointer or n < 0. */
int gpd_hip_shadow_jitter_model(uint64_t seed, const int32_t *voxels, int n, double *g);

/* The draws of SequentialImportanceSampling::detectGrasps (sequential_importance_sampling.cpp:189-270) — host only, no context;
 * the definition (gpd_amd/csrc/sis_model.h) the device draw of gpd_hip_detect_sis equals.  The reference draws from
 * std::random_device, rand() and static std::normal_distributions; here round r (0-based, after the initial pass) has two
 * xorshift64 streams (the one described at gpd_detect_job::num_draws), seeds in uint32 arithmetic: kind 0, the Gaussian
 * proposals, seed + 1000003 * (2r); kind 1, the uniform ones, seed + 1000003 * (2r + 1).
 * A Gaussian proposal takes 7 draws: idx_raw, then three offsets sigma * sqrt(-2 log u1) * cos(2 pi u2) of two draws each
 * (u1 = ((draw >> 11) + 1) / (2^53 + 1), u2 = (draw >> 11) / 2^53, the host's libm).  A uniform proposal is one draw, pos_raw.
 * gpd_hip_sis_proposals writes proposals first .. first + count of a stream: kind 0 into gpd_sis_proposal[count], kind 1 into
 * uint64_t[count] (sigma is not read).  GPD_ERR_INVALID: a NULL out with count > 0, a negative round / first / count, a kind
 * other than 0 or 1, sigma <= 0 for kind 0. */
typedef struct gpd_sis_proposal {
  uint64_t idx_raw;
  double off[3];
} gpd_sis_proposal;
int gpd_hip_sis_proposals(uint32_t seed, int round, int kind, long long first, int count, double sigma, void *out);

/* The selection rule over one block of each stream.  centres: the samples of the hand sets that keep a valid hand after
 * filterGraspsWorkspace (and the direction filter), in accumulated order, num_centres >= 1.
 *  - Gaussian: idx = idx_raw % num_centres, x = centre[idx] + off.  sampling_method 0 (SUM_OF_GAUSSIANS, :189-201) accepts every
 *    proposal; 1 (MAX_OF_GAUSSIANS, :203-237) accepts iff d2(x, centre[idx]) <= min over k of d2(x, centre[k]), d2 = (dx*dx + dy*dy)
 *    + dz*dz in double.  (The reference compares term * exp(-d2 / (2 sigma)) with >=: what is accepted here is accepted there.)
 *  - uniform: the point uniform_list[pos_raw % num_uniform_list] (uniform_list NULL: the point pos_raw % num_points) as the float
 *    coordinates of cloud_xyz cast to double, accepted iff inside workspace[6] with inclusive bounds (:263-265).
 *  - samples ((num_gauss + num_rand) x 3 doubles): the first num_gauss accepted Gaussian proposals in proposal order, then the
 *    first num_rand accepted uniform ones.
 * accepted[2] / consumed[2] (Gaussian, uniform) are in/out: zero them for a round's first blocks, pass them on unchanged with the
 * NEXT blocks of the streams when *shortfall (samples still missing) is > 0 — the result equals one long block.  consumed
 * counts the proposals up to and including the one that filled the list.
 * GPD_ERR_INVALID: a NULL argument that is needed, num_centres < 1 with num_gauss > 0, a method other than 0 or 1, an index of
 * uniform_list out of range. */
int gpd_hip_sis_select(const double *centres, int num_centres, const gpd_sis_proposal *gauss, int num_gauss_proposals,
                       const uint64_t *uniform, int num_uniform_proposals, const int32_t *uniform_list, int num_uniform_list,
                       const float *cloud_xyz, int num_points, const double *workspace, int sampling_method, int num_gauss, int num_rand,
                       double *samples, int32_t *accepted, int32_t *consumed, int *shortfall);

/* SequentialImportanceSampling::detectGrasps (sequential_importance_sampling.cpp:54-187) on the cloud uploaded last, the round
 * loop kept on the device:
 *  - the initial pass (:63-82) is the front half of gpd_hip_detect on sample_indices: index search, filterGraspsWorkspace, the
 *    direction filter when set, images of the valid hands;
 *  - round r (:95-160) draws num_samples samples around the live centres found so far (gpd_hip_sis_select on proposal blocks
 *    the host generates, applied by a kernel that writes the samples where the search reads them), searches them by
 *    coordinates (gpd_hip_search_samples' semantics) and appends live centres, candidate records and images to accumulators
 *    on the device.  set_index of a record is the index of its hand set in the accumulated live list; the order is round-major,
 *    set-major, slot-minor.  The shadow stream runs on through the rounds, so every hand set sits in it where ONE
 *    createImages over the whole list (:167) puts it.  Rounds end after num_iterations or when no live centre exists (:79-82);
 *  - ONE LeNet pass over all accumulated images (:164-167), in the context's LeNet mode; records with score > min_score (strict)
 *    are kept in order; with min_inliers > 0 they go through Clustering::findClusters (:175-181) and `hands` receives what
 *    gpd_hip_find_clusters returns on that list.
 * Per round only small words come back (the plan summary, the draw counts, the capacity flags); the records leave in one copy.
 * GPD_ERR_INVALID before any work: an index out of range, num_samples < 1 with num_iterations > 0, prob_rand_samples outside
 * [0, 1], sigma <= 0, a method other than 0 or 1, a NULL hands with capacity > 0, a negative count.  GPD_ERR_STATE: no cloud, no
 * weights, or a call while gpd_hip_detect_batch drives the lanes.  GPD_ERR_CAPACITY: capacity smaller than the result (num_hands
 * still says how many there were), centres_capacity smaller than the live list, or accumulators beyond 16 GB. */
typedef struct gpd_sis_job {                 /* zero it first */
  const int32_t *sample_indices;             /* in: the initial pass; also the source of the uniform proposals (cloud.getSampleIndices(), */
  int32_t num_init_samples;                  /*     :246-252); none: every point of the cloud is a uniform source                          */
  int32_t num_iterations;                    /* rounds after the initial pass */
  int32_t num_samples;                       /* samples per round */
  int32_t sampling_method;                   /* 0: SUM_OF_GAUSSIANS, 1: MAX_OF_GAUSSIANS */
  double prob_rand_samples;                  /* share of uniform samples per round: num_rand = (int)(prob * num_samples) */
  double sigma;                              /* standard deviation of the Gaussian offsets */
  double min_score;                          /* records are kept for score > min_score */
  double workspace[6];                       /* of the uniform proposals (cfg workspace) */
  int32_t min_inliers, remove_inliers;       /* clustering; min_inliers <= 0: none */
  uint32_t seed;
  int32_t proposal_block;                    /* proposals per stream and block; 0: sized from the acceptance rate so far */
  gpd_hand *hands;                           /* out: capacity records */
  int32_t capacity;
  int32_t num_hands;                         /* out: records written (GPD_ERR_CAPACITY: records there were) */
  int32_t rounds_run;                        /* out: rounds after the initial pass that ran */
  int32_t num_sets, num_candidates;          /* out: accumulated live hand sets / candidates */
  int32_t centres_capacity;                  /* in: centres centres_out can take */
  double *samples_out;                       /* out, may be NULL: num_iterations x num_samples x 3, the samples of every round run */
  double *centres_out;                       /* out, may be NULL: centres_capacity x 3, the accumulated live centres */
  int32_t *round_counts;                    /* out, may be NULL: (1 + num_iterations) x {live sets, candidates, Gaussian proposals
                                                consumed, uniform proposals consumed}; row 0 is the initial pass */
  int64_t d2h_bytes;                         /* out: bytes this call copied device -> host */
  float stage_ms[4];                         /* out: draw, search, images + accumulate, LeNet + select + cluster (HIP events) */
} gpd_sis_job;
int gpd_hip_detect_sis(gpd_hip_ctx *ctx, gpd_sis_job *job);
int gpd_hip_sizeof_sis_job(void);

/* Replaces ImageGenerator::createImages (image_generator.cpp:17-99) for hand
 * sets produced by the last gpd_hip_search / gpd_hip_detect on this context (optionally after
 * the host filters, grasp_detector.cpp:334-398 / :422-453, which clear `valid`: only the `valid`
 * flags and the sets' samples are read from `hands`, the records themselves are on the device).  One image per valid hand
 * in set-major, slot-minor order; sets without a valid hand are skipped like
 * filterGraspsWorkspace drops them.  images (may be NULL: keep on device) holds
 * n_cand * 60*60*C bytes HWC.  cand_index (may be NULL) receives for each image
 * the index into `hands`. */
int gpd_hip_images(gpd_hip_ctx *ctx, const gpd_hand *hands, int num_sets,
                   uint8_t *images, int32_t *cand_index, int *num_candidates);

/* Hand sets the CALLER supplies — from another sampler, a file, an earlier frame, a perturbation of a good grasp, a list
 * gathered over several searches — instead of the last search's: ImageGenerator::createImages(cloud, hand_set_list)
 * (image_generator.cpp:17-99) images whatever it is handed.
 *
 * gpd_hip_given_check (host only, no context; the definition is csrc/given_model.h): what may be supplied.  The layout is
 * gpd_hip_images': num_sets x slots records, set-major, slots = num_hand_axes * num_orientations.  A set's sample is slot 0's
 * `sample` and must be finite even when slot 0 is not valid.  Every record with valid != 0 must have
 *   - `sample` equal to the set's sample bit for bit (the reference's HandSet has one sample),
 *   - finite `frame`, `bottom`, `center`; `frame` a rotation: every entry of F^T F - I within 1e-6,
 *   - init_bite - hand_depth <= bottom <= 0 and |center| <= (hand_outer_diameter - finger_width) / 2, each with 1e-9 of slack:
 *     the ranges the voxel windows of the image kernels are sized for (hands outside them are refused, not routed elsewhere).
 * Records with valid == 0 are husks: nothing but slot 0's sample is read from them.  GPD_ERR_INVALID outside that domain, the
 * first offending set / slot in *bad_set / *bad_slot (may be NULL; -1 / -1 on GPD_OK), the reason in gpd_hip_last_error().
 *
 * gpd_hip_images_given: the images of such hand sets on the context's uploaded cloud.  A set's image neighbourhood is the
 * nn_radius_images sphere around the float cast of its sample, in (d2, index) order; sets without a valid hand are skipped and
 * consume no shadow draws, the others take their place in the one shadow LCG stream in the order given, starting at lcg_base
 * (0: a whole cloud); candidates are the valid hands, set-major and slot-minor.  Every set is a set: no frame is estimated and
 * no hand evaluated here, so a sample without a point inside nn_radius_frames is kept.  images (may be NULL: keep on the device,
 * for gpd_hip_score(ctx, NULL, n, ...)), cand_index, num_candidates as gpd_hip_images; lcg_draws (may be NULL): the shadow draws
 * the sets consumed.
 *
 * gpd_hip_score_given: the same followed by the LeNet in the context's mode and ReLU setting.  `score` of every valid record is
 * written; no other byte of `hands` changes.  scores (may be NULL): one per candidate.
 *
 * Both reuse the search buffers, as gpd_hip_reevaluate does: hands of an earlier gpd_hip_search can no longer be passed to
 * gpd_hip_images afterwards.  GPD_ERR_STATE without a cloud (or weights, for the scoring entry); GPD_ERR_INVALID from the
 * check, made before anything is enqueued: the context is as it was. */
int gpd_hip_given_check(const gpd_params *params, const gpd_hand *hands, int num_sets, int *bad_set, int *bad_slot);
int gpd_hip_images_given(gpd_hip_ctx *ctx, const gpd_hand *hands, int num_sets, uint64_t lcg_base, uint8_t *images,
                         int32_t *cand_index, int *num_candidates, uint64_t *lcg_draws);
int gpd_hip_score_given(gpd_hip_ctx *ctx, gpd_hand *hands, int num_sets, uint64_t lcg_base, float *scores, int32_t *cand_index,
                        int *num_candidates, uint64_t *lcg_draws);

/* Fused path used by GraspDetector::detectGrasps steps 1-4
 * (grasp_detector.cpp:222-273): search, workspace/aperture filter
 * (filterGraspsWorkspace, :238, :334-398), images, scores, score write-back (:269-273).
 * Everything stays on the device between the stages: the filter runs at the end of the
 * hand kernel, one small kernel builds the candidate list (set-major, slot-minor, as
 * image_generator.cpp:91-98) and places every hand set in the shadow LCG stream, and the
 * only host hop in the middle is a 48-byte summary that sizes the launches.  One copy in
 * (the samples), one copy out (the records).  hands receives num_sets*num_slots records
 * (room for num_samples*num_slots is required): `valid` is the flag after the filter,
 * `score` is set on the valid ones. */
int gpd_hip_detect(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples,
                   gpd_hand *hands, int *num_sets, int *num_candidates);

/* The same, returning what detectGrasps keeps after step 4 / step 5 instead of every slot:
 * num_selected == 0: the scored candidates — the `hands` list ImageGenerator::createImages moves
 *   out of the hand sets (image_generator.cpp:91-98), in that order;
 * num_selected  > 0: GraspDetector::selectGrasps (grasp_detector.cpp:405-420): the
 *   min(num_selected, candidates) best, score descending, picked on the device so that only those
 *   records cross PCIe (equal scores: the arrangement std::partial_sort leaves, as the reference).
 * hands holds hands_capacity records; *num_hands receives how many were written. */
int gpd_hip_detect_select(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples, int num_selected,
                          gpd_hand *hands, int hands_capacity, int *num_sets, int *num_candidates,
                          int *num_hands);

/* Sizes every buffer of the context — both lanes of the batch entry — for clouds of up to max_points points,
 * max_cams cameras and max_samples samples, so that no later call within those sizes allocates (growing a buffer is
 * a hipFree + hipMalloc, which waits for the whole device).  max_candidates: scored hands per cloud, 0 = the upper
 * bound max_samples x slots (cut to 16 GB of candidate-sized buffers per lane); max_selected: the largest
 * num_selected that will be asked for (0: none).  Optional: gpd_hip_detect_batch sizes its lanes itself from the
 * jobs it is given; the single-cloud entries grow their buffers on demand (25 % slack, never shrinking).  The scoring
 * scratch is that of the network the context holds NOW: with one installed by gpd_hip_set_lenet_net, the general route's
 * (a candidate priced at its scratch bytes per image, gpd_hip_lenet_net_info) and one image's worth of the stock one; call
 * this after the install, a later install frees that scratch again.  No reference counterpart: the reference allocates per
 * call. */
int gpd_hip_reserve(gpd_hip_ctx *ctx, int max_points, int max_cams, int max_samples, int max_candidates, int max_selected);

/* One independent cloud of a batch: the arguments of gpd_hip_upload_cloud + gpd_hip_detect_select.
 * ZERO the struct (memset / `gpd_detect_job j = {0}`) before filling it: fields added in later rounds (lcg_base, raw, voxel_size,
 * workspace, normals_radius, sample_xyz, refine_normals_k, sample_above_plane, num_draws, sample_seed, samples_out, outlier_mean_k, outlier_stddev_mult) are INPUTS,
 * and an uninitialised `raw` or `lcg_base` selects the raw-scan route or offsets the cloud's shadow stream — wrong images, not an
 * error; an uninitialised `num_draws` or `samples_out` of a raw job draws samples nobody asked for or writes through a wild pointer. */
typedef struct gpd_detect_job {
  const float *xyz;            /* in */
  const float *normals;
  const int32_t *cam_source;
  const double *view_points;
  const int32_t *sample_indices;
  gpd_hand *hands;             /* out: hands_capacity records */
  int32_t num_points, num_cams, num_samples;
  int32_t num_selected;        /* 0: all candidates; > 0: selectGrasps */
  int32_t hands_capacity;
  int32_t num_sets, num_candidates, num_hands; /* out */
  int32_t status;              /* out: GPD_OK or the error of this cloud */
  float stage_ms[3];           /* out: search, images, LeNet kernel time of this cloud */
  /* out: where the HOST was, in ms since the entry of gpd_hip_detect_batch: [0] upload + search + plan enqueued,
   * [1] plan summary arrived (the only mid-pipeline wait), [2] images + LeNet + gather enqueued, [3] results on the
   * host, [4] records handed over.  A host-side limiter shows here, not in stage_ms. */
  float host_ms[5];
  int32_t allocs;              /* out: buffer growths (hipFree + hipMalloc = a device stall) booked on this cloud;
                                  0 everywhere but the first cloud of a batch whose lanes were not yet sized */
  int32_t reserved_;
  /* The cloud's ONE stream of shadow draws (HandSet::fastrand, hand_set.cpp:263-283) when its samples are cut into ranges:
   * lcg_base (in) = draws of the sample ranges before this job's (0: the job starts the cloud's stream — every ordinary
   * call), lcg_draws (out) = draws of this job's hand sets.  gpd_hip_detect_sharded fills lcg_base itself. */
  uint64_t lcg_base;
  uint64_t lcg_draws;
  /* RAW scans (round 5): raw != 0 -> xyz / cam_source are the cloud as detect_grasps reads it from the sensor or the PCD, and
   * the job runs CandidatesGenerator::preprocessPointCloud (candidates_generator.cpp:14-37) on the device first:
   * Cloud::filterWorkspace with `workspace` (6 doubles xmin xmax ymin ymax zmin zmax; NULL: none), Cloud::voxelizeCloud
   * (voxel_size; <= 0: none), Cloud::calculateNormals(normals_radius, towards the cameras that see each point).  `normals` and
   * `sample_indices` are ignored (indices into the preprocessed cloud do not exist yet): the search runs at `sample_xyz`
   * (num_samples x 3 doubles, the `samples` route of the reference: cloud.h setSamples, hand_search.cpp:160-165).  The voxelised
   * cloud never leaves the device; the voxeliser's sequential keep / drop chain runs on the calling host thread while the
   * previous cloud's image / LeNet kernels run.  num_points_processed (out): points after preprocessing.
   * As in the reference, the preprocessing starts with Cloud::removeNans (a point with a NaN / Inf coordinate is dropped — the rows
   * an organised sensor scan carries for missing depth) and Cloud::filterWorkspace cuts the SAMPLES too (cloud.cpp:225-237: strict
   * double comparisons, order kept): the search runs at the samples inside `workspace` only, num_samples_processed (out) says how
   * many those were, and the job's records are those of that many samples. */
  int32_t raw;
  float voxel_size;
  const double *workspace;
  double normals_radius;
  const double *sample_xyz;
  int32_t num_points_processed;
  int32_t num_samples_processed;
  /* The rest of preprocessPointCloud for a RAW scan (candidates_generator.cpp:28-36); read only when raw != 0, all zero: as above.
   * refine_normals_k (in) > 0: Cloud::refineNormals(k) after the normals (cloud.cpp:176-204) with the reference's fixed settings —
   *   15 passes at most, convergence threshold 1e-5f — as gpd_hip_refine_normals; the search reads the refined normals.
   *   k > 256: GPD_ERR_CAPACITY, k < 0: GPD_ERR_INVALID, for this job alone.
   * The INDEX route — sample_xyz == NULL, num_samples == 0, num_draws > 0 — is detect_grasps on a PCD file without samples:
   *   sample_above_plane (in) != 0: Cloud::sampleAbovePlane() (cloud.cpp:407-436) with the reference's values (0.01, 50, 0.99,
   *     optimize) as gpd_hip_sample_above_plane: the candidate list is the points off the support plane, ascending; a failed fit
   *     (plane_num_above == 0) leaves none, and as in the reference the whole cloud is used then.
   *   num_draws, sample_seed (in): Cloud::subsample(num_draws) (cloud.cpp:350-405) on the project's seeded stream (xorshift64 from
   *     0x9E3779B97F4A7C15 ^ sample_seed, steps << 13, >> 7, << 17 — the reference's generators are time-seeded).  With a list of n
   *     entries: num_draws >= n keeps the whole list in order, otherwise num_draws draws WITH repetition, list[next() % n].  Without
   *     a list: a partial Fisher-Yates over the M preprocessed points, min(num_draws, M) distinct indices.
   *     gpd_hip_sample_positions gives the positions on the host.
   *   samples_out (in; may be NULL, else room for num_draws entries): receives the sample indices into the preprocessed cloud the
   *     search ran at, num_samples_processed of them.  The list, the draw and the search stay on the device: a few KB of positions
   *     go up, this copy comes down.
   *   num_samples_processed, num_sets, num_candidates, lcg_draws follow as on any index search; the lanes are sized with num_draws
   *   as the sample count (the number searched never exceeds it).
   * The COORDINATES route (sample_xyz given) is the one above plus the refinement when asked for.  sample_above_plane is accepted
   *   there and changes nothing: HandSearch::searchHands reads the samples before the sample indices (hand_search.cpp:37-39) and
   *   sampleAbovePlane only rewrites the latter, so the fit is not run and the plane_* outputs stay 0; samples_out is not written.
   *   num_draws != 0 together with sample_xyz is GPD_ERR_INVALID for this job (the two sampling modes are not mixed), so is
   *   num_draws < 0.  With num_draws == 0 and no samples nothing is searched and the fit is not run.
   * A job that fails here carries its own status; the batch goes on. */
  int32_t refine_normals_k;
  int32_t sample_above_plane;
  int32_t num_draws;
  uint32_t sample_seed;
  int32_t *samples_out;
  int32_t refine_passes;     /* out: passes the refinement ran (0: not asked for) */
  int32_t refine_num_nan;    /* out: refined normals with a non-finite component */
  int32_t plane_num_above;   /* out: points off the support plane; 0: the fit failed or was not run */
  int32_t plane_iterations;  /* out: hypotheses RANSAC evaluated */
  float preprocess_ms[4];    /* out: host wall time of this job's cut + voxeliser, normals, refinement, plane fit */
  /* Cloud::removeStatisticalOutliers for a RAW scan (read only when raw != 0; zero: off, as above): outlier_mean_k (in) > 0 runs
   * gpd_hip_remove_statistical_outliers(outlier_mean_k, outlier_stddev_mult) AFTER the voxeliser and BEFORE calculateNormals — the
   * reference gives the method no position (it never calls it); this is the one place where the cloud that the normals, the
   * search and the images see has a grid.  num_points_processed then counts the kept points, the index route draws from them,
   * and the kept cloud never leaves the device.  outlier_mean_k < 0, a non-finite outlier_stddev_mult or fewer than
   * outlier_mean_k + 1 points after the voxeliser: GPD_ERR_INVALID; outlier_mean_k > 255: GPD_ERR_CAPACITY — for this job alone. */
  int32_t outlier_mean_k;
  int32_t num_outliers;      /* out: points the step removed (0: not asked for) */
  double outlier_stddev_mult;
  float outlier_ms;          /* out: host wall time of the step */
  int32_t reserved2_;
} gpd_detect_job;

/* The positions Cloud::subsample draws from a candidate list of n entries on the seeded stream described at
 * gpd_detect_job::num_draws — host only, no context.  with_repetition != 0: the list is a cloud's sample indices
 * (num_draws >= n: 0 .. n-1 in order, else num_draws draws next() % n); 0: the list is the cloud's n points (the first
 * min(num_draws, n) entries of a Fisher-Yates shuffle, distinct; computed with a sparse swap map, so n may be large).
 * out holds max(min(num_draws, n), 0) entries; *num_out receives how many were written (num_draws <= 0: none).
 * GPD_ERR_INVALID: n < 0 or a NULL num_out / out. */
int gpd_hip_sample_positions(int n, int num_draws, uint32_t seed, int with_repetition, int32_t *out, int *num_out);

/* detect_grasps over a batch of independent clouds (src/detect_grasps.cpp:20-86 called once per
 * cloud; BASELINE configs[4]).  The context keeps two clouds in flight on two streams: upload, grid
 * and candidate search of cloud i+1 are enqueued while the image and LeNet kernels of cloud i run,
 * and the records of cloud i-1 are handed over meanwhile — the host hops of one cloud hide behind
 * the kernels of its neighbour.  Results are those of num_jobs separate
 * gpd_hip_upload_cloud + gpd_hip_detect_select calls (the shadow LCG restarts per cloud).  Returns
 * the first error; each job carries its own status.  The cloud uploaded with gpd_hip_upload_cloud
 * is replaced. */
int gpd_hip_detect_batch(gpd_hip_ctx *ctx, gpd_detect_job *jobs, int num_jobs);

/* The same over several contexts — one per GPU of a node, one host thread per context, job i -> context
 * i mod num_ctx, no device talks to another ("one host thread + one gpd_hip_ctx + 2-3 streams per
 * GPU"; the reference's unit of work is one detect_grasps process per cloud, src/detect_grasps.cpp:20-86).
 * Every context must carry the LeNet weights.  Results are those of gpd_hip_detect_batch on any one context
 * (the shadow LCG restarts per cloud, so they do not depend on the sharding).  Returns the first error. */
int gpd_hip_detect_batch_multi(gpd_hip_ctx *const *ctxs, int num_ctx, gpd_detect_job *jobs, int num_jobs);

/* ONE cloud over several contexts ("sample-range sharding with the cloud replicated"; BASELINE configs[3] across
 * GPUs): shards[g] is the job of ctxs[g] — the same cloud arrays, a CONTIGUOUS range of the cloud's samples (range g before
 * range g + 1 in the caller's sample order), its own output buffer, num_selected = 0.  The reference draws all shadow points of a
 * cloud from one LCG stream, hand set after hand set (hand_set.cpp:268-283): phase 1 searches every range and takes its draw
 * total, the totals are scanned on the host (num_ctx numbers — still no collective), phase 2 generates and scores the images
 * with lcg_base = the draws of the ranges before.  The concatenated records are byte for byte those of ONE
 * gpd_hip_detect_select(num_selected = 0) over all samples, whatever the split.  Every context must carry the LeNet weights. */
int gpd_hip_detect_sharded(gpd_hip_ctx *const *ctxs, int num_ctx, gpd_detect_job *shards);

/* Binds the CALLING host thread to the CPUs of the NUMA node `device` hangs off (sysfs numa_node / cpulist, within the
 * process's allowed set): the thread that feeds a GPU — staging copies, launches, result copies — should run on that
 * GPU's socket (8 feeding processes on a two-socket host).  Returns the node, or -1 when the host exposes no
 * topology (nothing changed); *num_cpus (may be NULL) receives the size of the new mask.  gpd_hip_detect_batch_multi does
 * this for its worker threads; one-process-per-GPU launchers (bench.py) call it before gpd_hip_create.  Pinned staging
 * memory is placed by hipHostMalloc near the current device already.  No reference counterpart. */
int gpd_hip_bind_host_thread(int device, int *num_cpus);

/* gpd_hip_detect for samples given by coordinates (see gpd_hip_search_samples). */
int gpd_hip_detect_samples(gpd_hip_ctx *ctx, const double *samples_xyz, int num_samples,
                           gpd_hand *hands, int *num_sets, int *num_candidates);

/* Stage times of the last call in milliseconds (HIP events on the context's
 * stream): [0] search, [1] images (incl. shadow), [2] score.  The counterpart
 * of the RUNTIMES printout, grasp_detector.cpp:313-320. */
int gpd_hip_last_stage_ms(gpd_hip_ctx *ctx, float ms[3]);

/* Sizes of the last gpd_hip_images call, for the algorithmic byte count of SURVEY §8d:
 * out[0] candidates, out[1] live hand sets, out[2] sum over live sets of the image
 * neighbourhood size N_i, out[3] sum over candidates of N_i. */
int gpd_hip_last_images_stats(gpd_hip_ctx *ctx, long long out[4]);

/* Which slow paths the last search / image stage took (none of them changes a result):
 * out[0] entries per neighbourhood list the search ran with (8192: bucket sort in LDS; 16384: bitonic sort in LDS;
 * more: global-memory lists), out[1] candidates whose box held more shadow voxels than the two-per-CU shadow
 * kernel lists (redone by the large instantiation), out[2] candidates with more in-box points than the two-per-CU
 * normals/depth kernel holds (redone with global scratch), out[3] LeNet passes of the last scoring (65536 images
 * each).  Waits for the context's stream. */
int gpd_hip_last_fallbacks(gpd_hip_ctx *ctx, long long out[4]);

/* Which image kernels the last image launch of the single-cloud entries (gpd_hip_images, gpd_hip_detect*, gpd_hip_replay)
 * sent each candidate through, read back from the device lists the kernels fill (none of it changes a result).
 * Tests only: the timed path never calls it.  Waits for the context's stream.
 * route (n entries, n >= info[0]): per candidate of the launch, in candidate order, a bit mask —
 *   1: the two-per-CU shadow kernel could not list its box and queued it for the large instantiation,
 *   2: the large one (wide windows) could not list it either and queued it for the general shadow kernel,
 *   4: the two-per-CU normals / depth kernel queued it for the global-scratch instantiation;
 *   0: its images came from the first kernel of each kind alone (window class 2: the general shadow kernel takes all).
 * info: [0] candidates of the launch, [1] window class of the geometry (0 default, 1 wide, 2 huge), [2] the
 * shadow_set_kernel mode that ran (0, 1, 2; -1: none), [3] the capacity flags of the launch (1 window, 2 in-box points,
 * 4 in-box shadow voxels: what GPD_ERR_CAPACITY reports), [4] PT_CAP, [5] PT_CAP_BIG, [6] SH_CAP, [7] SH_CAP_BIG.
 * GPD_ERR_INVALID for a null argument or n < info[0]; GPD_ERR_STATE if a list holds an entry that is no candidate. */
int gpd_hip_last_image_routes(gpd_hip_ctx *ctx, int32_t *route, int n, long long info[8]);

/* Which route every point took through the last gpd_hip_estimate_normals of the context, read back from what its kernels left
 * on the device (none of it changes a result).  Tests only: the timed path never calls it.  Waits for the context's stream.
 * count (n entries, n >= info[0]): per point, by ORIGINAL index, the neighbours found within the radius, the point itself
 * included.  The count decides the route: up to 256 / 512 / 1024 a wave sorts the list in 4 / 8 / 16 registers per lane; beyond
 * 1024 the point is queued for the workgroup-per-point kernel, which sorts 2^ceil(log2 count) keys in LDS (up to 8192) or in
 * the point's slice of the arena.
 * info: [0] points, [1] tiles of 65536 cell-order positions the run took, [2] queued points, [3] of these, sorted in LDS,
 * [4] sorted in the arena, [5] attempts (2: the arena was too small, grew, and the run was repeated), [6] the arena's
 * capacity after the call in 8-byte slots, [7] points that were not queued and whose centroid could not be certified
 * order-free by the list kernel (their three fp64 chains were walked in neighbour order).
 * GPD_ERR_INVALID for a null argument or n < info[0]; GPD_ERR_STATE when no gpd_hip_estimate_normals ran on the cloud the
 * context holds (an upload, or another entry that replaces the cloud or its normals, came after it). */
int gpd_hip_last_normals_routes(gpd_hip_ctx *ctx, int32_t *count, int n, long long info[8]);

/* Of the last search's 3 x num_samples centre coordinates (the mean of a sample's image neighbourhood, hand_set.cpp:131-133):
 * how many took the serial fp64 chain in neighbour order because the order-free sum taken inside the neighbourhood kernel could
 * not be certified exact (a point within micrometres of a coordinate plane among points decimetres away).  Wherever the
 * certificate holds the sum is the same in EVERY order — the oracle's sequential one and Eigen's packet reduction alike.
 * Measurement / tests only.  Waits for the context's stream. */
int gpd_hip_last_centre_chains(gpd_hip_ctx *ctx, long long *out);

/* Re-run stage 3 (stages == 1: grasp images), stage 4 (2: LeNet) or both (3) on the
 * candidate list that the last gpd_hip_images / gpd_hip_detect left resident on the
 * device — what calling ImageGenerator::createImages + Classifier::classifyImages
 * again on the same hand sets does (grasp_detector.cpp:261-273), without host hops.
 * Asynchronous on the context's stream; each call is bracketed by HIP events. */
int gpd_hip_replay(gpd_hip_ctx *ctx, int stages);

/* Synchronise; ms[0] / ms[1] = summed HIP-event time of the image / LeNet stage over the
 * gpd_hip_replay calls since the last query, *launches = their number; scores (may be
 * NULL) receives the scores of the last replay. */
int gpd_hip_replay_times(gpd_hip_ctx *ctx, float ms[2], int *launches, float *scores);

/* HIP-event durations of the four LeNet kernels (conv1+pool1, conv2+pool2, ip1, ip2+score; first
 * 65536-image chunk) summed over the replays covered by the last gpd_hip_replay_times call —
 * the per-kernel roofline input of bench.py. */
int gpd_hip_replay_kernel_ms(gpd_hip_ctx *ctx, float ms[4]);

/* conv1's zero skipping, counted by the kernel itself: pairs[0] = (64-pixel chunk, channel) pairs it executed,
 * pairs[1] = pairs it looked at, summed over the launches on the context's first lane since the last reset.
 * executed / looked-at x the dense FLOP count = the FLOPs the matrix pipe really ran (rounds 1-4: bench.py's roofline.frac).
 * GPD_LENET_F32_CHAIN only — the split conv1 executes every tile and counts nothing (both numbers stay 0).
 * Measurement only: no reference counterpart. */
int gpd_hip_conv1_stats(gpd_hip_ctx *ctx, unsigned long long pairs[2], int reset);
/* test hook: intermediate tensors of the last gpd_hip_score pass (n images; after the conv ReLU when gpd_hip_set_lenet_conv_relu is
 * on) — which = 0: pool1 f32 [n][15680] (layout of the
 * mode), 1: the three bf16 planes of the flattened pool2 [3][n][7200] (GPD_LENET_SPLIT; un-blocked on the host), 2: ip1 after ReLU, transposed f32 [500][n]
 * (GPD_LENET_SPLIT: the four K-quarter partial sums added on the host as ip2's kernel adds them) */
int gpd_hip_lenet_debug(gpd_hip_ctx *ctx, int which, int n, void *out);
/* test hook, host only: the operand tables of the split path's conv kernels as uploaded — atab: conv1's int8 digit
 * fragments [7][5][64][16], corr / shift [20], btab: conv2's bf16 fragments [4 slots][3][16][64][8] (slots 0-2: filters 16 slot + lane % 16; slot 3, k-steps 0-3: the
 * (filter, kernel column) rows of filters 48 and 49) */
int gpd_hip_lenet_fast_tables(int channels, const float *conv1_w, const float *conv2_w, uint8_t *atab, double *corr, int *shift,
                              unsigned short *btab);

/* ---- training (train.hip) ----------------------------------------------------------------------------------
 * A trainer for pytorch/network.py::Net as pytorch/train_net3.py trains it: softmax cross-entropy (mean over the batch) and
 * torch.optim.Adam with weight_decay as L2 (g + wd * p), all in f32, every sum in a fixed order: two runs from the same state,
 * data and index lists give the same bytes.  The state is exchanged as the eight tensors of the state dict in torch layout, in
 * this order: conv1.weight [20][C][5][5], conv1.bias [20], conv2.weight [50][20][5][5], conv2.bias [50], fc1.weight [500][7200],
 * fc1.bias [500], fc2.weight [2][500], fc2.bias [2] — what gpd_hip_lenet_from_torch takes. */
typedef struct gpd_train_params {
  int32_t channels;     /* 1, 3, 12 or 15 */
  int32_t max_batch;    /* 1 .. 1024: every buffer is sized for it at creation */
  double lr, beta1, beta2, eps, weight_decay; /* torch.optim.Adam; train_net3.py: 1e-3, 0.9, 0.999, 1e-8, 5e-4 */
  double input_scale;   /* images enter as u8 * input_scale (hdf5_dataset.py:17: 1/256) */
} gpd_train_params;
typedef struct gpd_hip_trainer gpd_hip_trainer;

void gpd_hip_train_default_params(gpd_train_params *p); /* 15 channels, max_batch 64, the values above */
/* The trainer lives on the context's device and stream and must be destroyed before the context.  GPD_ERR_INVALID: a null
 * pointer, channels not in {1, 3, 12, 15}, max_batch outside 1 .. 1024, a non-finite or out-of-range hyper-parameter. */
int gpd_hip_train_create(gpd_hip_ctx *ctx, const gpd_train_params *params, gpd_hip_trainer **out);
void gpd_hip_train_destroy(gpd_hip_trainer *t);
/* Host only: every tensor U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (fan_in 25 C, 500, 7200, 500; a bias has its layer's) — the
 * distribution of torch's default initialisation, drawn from the project's seeded xorshift64 stream (sample_model.h), the eight
 * tensors in order; NOT torch's bits. */
int gpd_hip_train_init_state(int channels, uint32_t seed, float *const tensors[8]);
/* set: also clears Adam's moments and the step count; GPD_ERR_INVALID (nothing changed) for a non-finite value. */
int gpd_hip_train_set_state(gpd_hip_trainer *t, const float *const tensors[8]);
int gpd_hip_train_get_state(gpd_hip_trainer *t, float *const tensors[8]);
/* The resident set `which` (0: training, 1: test): images u8 [n][60][60][C] HWC, labels u8 [n] (0 / 1, GPD_ERR_INVALID
 * otherwise).  n = 0 clears the slot.  GPD_ERR_CAPACITY: more than 4 GiB of images in one slot. */
int gpd_hip_train_set_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n);
/* A resident set is a pool: n images in room for `capacity`, which grows.  Pools carry no 4 GiB limit (gpd_hip_train_set_data
 * keeps its own); the image count is an int, every byte offset 64 bits wide.  Each entry below synchronises the trainer's
 * stream before it moves or frees a pool, and returns after its copies and kernels have completed.
 *  - reserve: room for exactly max(capacity_images, n) images, the n images of the set kept (moved device to device when the
 *    pool is reallocated).  GPD_ERR_CAPACITY: the device has no such room; the pool is as it was.
 *  - count: *n images, room for *capacity (may be NULL).
 *  - append_data: n host images and labels behind the set's last image; labels checked as set_data checks them (nothing
 *    changes on GPD_ERR_INVALID).  A pool that is too small grows to max(need, 1.5 x capacity).  A set made by set_data can be
 *    appended to.
 *  - get_data: images [first, first + count) and their labels to the host.  GPD_ERR_INVALID: a range outside [0, n).
 *  - reorder: images and labels of [first, first + count) become new[k] = old[first + order[k]], by a copy of the range to a
 *    scratch block and a gather back on the device.  GPD_ERR_INVALID (nothing changed): a range outside [0, n), or an order
 *    that is no permutation of 0 .. count - 1 (checked on the host). */
int gpd_hip_train_reserve(gpd_hip_trainer *t, int which, int capacity_images);
int gpd_hip_train_count(gpd_hip_trainer *t, int which, int *n, int *capacity);
int gpd_hip_train_append_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n);
int gpd_hip_train_get_data(gpd_hip_trainer *t, int which, int first, int count, uint8_t *images_hwc, uint8_t *labels);
int gpd_hip_train_reorder(gpd_hip_trainer *t, int which, int first, int count, const int32_t *order);
/* gpd_hip_label_view whose kept instances never leave the device: the rounds and the balance selection of `job` run on `ctx`
 * (the trainer's own context or another one on the same device, with the trainer's channel count: GPD_ERR_INVALID before any
 * work otherwise), and the gather writes the kept images and labels straight behind the n images of set `which`, the pool grown
 * first when needed.  job->images, labels, hands, src_index and capacity are not read; all_labels, round_counts, the counters and
 * stage_ms are gpd_hip_label_view's; d2h_bytes holds no image byte (plan summaries, counts, all_labels).  The first appended
 * image is at the n gpd_hip_train_count returned before the call, num_out images follow.  Returns after the gather has
 * completed; on any error n is unchanged.  Errors beyond these: gpd_hip_label_view's. */
int gpd_hip_train_append_view(gpd_hip_trainer *t, int which, gpd_hip_ctx *ctx, gpd_label_view_job *job);
/* num_steps Adam steps on the training set, step s on the images indices[s * batch .. (s + 1) * batch), 1 <= batch <= max_batch;
 * losses [num_steps]: each step's loss before its update.  The steps are enqueued back to back and waited for once (calls
 * with more than 2^20 indices: once per 2^20).  GPD_ERR_INVALID before anything is launched: an index outside [0, n). */
int gpd_hip_train_steps(gpd_hip_trainer *t, const int32_t *indices, int num_steps, int batch, float *losses);
/* Forward and backward of one batch with no update: grads as the eight tensors, the loss. */
int gpd_hip_train_gradients(gpd_hip_trainer *t, const int32_t *indices, int batch, float *const grads[8], float *loss);
/* One Adam step from gradients of the host's (non-finite values: GPD_ERR_INVALID). */
int gpd_hip_train_apply(gpd_hip_trainer *t, const float *const grads[8]);
/* Forward only over set `which`: images indices[0 .. n), or 0 .. n - 1 for indices == NULL -> logits [n][2], the number of rows
 * whose first maximum (torch.max) is the label. */
int gpd_hip_train_eval(gpd_hip_trainer *t, int which, const int32_t *indices, int n, float *logits, int *num_correct);
/* Measurement only: one training step with a HIP event behind every kernel -> ms [*num] in launch order, names
 * gpd_hip_train_kernel_name(i); capacity: ms holds that many. */
int gpd_hip_train_step_timed(gpd_hip_trainer *t, const int32_t *indices, int batch, float *ms, int capacity, int *num);
const char *gpd_hip_train_kernel_name(int i);

/* ---- a second recipe: the deployed LeNet under Caffe's solver -----------------------------------------------
 * network 1 is the network the context scores by default — EigenClassifier's, models/caffe/15channels/
 * lenet_15_channels_train_val.prototxt: conv, 2x2 max-pool twice with NO ReLU behind the convolutions, fc1 (ip1), ReLU, fc2
 * (ip2), SoftmaxWithLoss.  solver 1 is Caffe's SGDSolver, per tensor t and in f32:
 *     d = g + (weight_decay * decay_mult[t]) * w;   h = momentum * h + (lr_s * lr_mult[t]) * d;   w = w - h
 * with params->lr as base_lr and params->weight_decay as weight_decay (beta1, beta2 and eps are ignored); L2 decay reaches the
 * biases too unless decay_mult says otherwise, lr_mult[t] = 0 freezes tensor t.  lr_s is the learning rate of the step's
 * 0-based update count `it` since the last gpd_hip_train_set_state (gpd_hip_train_learning_rate): evaluated on the host in
 * double, rounded to float once, handed to the step's launch.  Under solver 0 (Adam) the policy scales lr the same way (in
 * double; "fixed" is today's trainer to the byte) and multipliers other than 1 are refused. */
enum { GPD_TRAIN_NET_TORCH = 0, GPD_TRAIN_NET_CAFFE = 1 };
enum { GPD_TRAIN_SOLVER_ADAM = 0, GPD_TRAIN_SOLVER_SGD = 1 };
enum { GPD_LR_FIXED = 0, GPD_LR_STEP = 1, GPD_LR_EXP = 2, GPD_LR_INV = 3 };
#define GPD_TRAIN_CAFFE_BASE_LR 0.01 /* lenet_solver_15_channels.prototxt: base_lr, for gpd_train_params.lr */
typedef struct gpd_train_recipe {
  int32_t network;      /* GPD_TRAIN_NET_* */
  int32_t solver;       /* GPD_TRAIN_SOLVER_* */
  double momentum;      /* [0, 1); solver 1 only */
  int32_t lr_policy;    /* GPD_LR_*: fixed lr; step lr * gamma^floor(it / stepsize); exp lr * gamma^it; inv lr * (1 + gamma * it)^-power */
  int32_t stepsize;     /* >= 1 under step */
  double gamma, power;
  double lr_mult[8], decay_mult[8]; /* Caffe's param { lr_mult decay_mult }, the eight tensors in state order */
} gpd_train_recipe;
int gpd_hip_sizeof_train_recipe(void);
/* which = 0: today's trainer (Net, Adam, fixed, multipliers 1).  which = 1: the two prototxt files — the Caffe network, SGD
 * with momentum 0.9, inv with gamma 1e-4 and power 0.75, multipliers 1; their base_lr 0.01 and weight_decay 5e-4 belong in
 * gpd_train_params (GPD_TRAIN_CAFFE_BASE_LR; the default weight_decay is the solver file's already), max_iter 10000 and the
 * batch of 64 in the caller's loop.  Anything else: GPD_ERR_INVALID. */
int gpd_hip_train_default_recipe(gpd_train_recipe *r, int which);
/* gpd_hip_train_create with a recipe; NULL is gpd_hip_train_create.  GPD_ERR_INVALID beyond gpd_hip_train_create's: an unknown
 * network, solver or policy, a non-finite or negative multiplier, a multiplier other than 1 under Adam, momentum outside
 * [0, 1), stepsize < 1 under step, a non-finite gamma or power, a negative gamma under inv. */
int gpd_hip_train_create_recipe(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, gpd_hip_trainer **out);
/* Host only: Caffe's "xavier" filler as the train_val prototxt asks for it — weights U(-sqrt(3 / fan_in), sqrt(3 / fan_in)),
 * fan_in 25 C, 500, 7200, 500, biases 0 — from the project's seeded xorshift64 stream like gpd_hip_train_init_state (the
 * weight tensors in order, no draw for a bias); NOT Caffe's bits.  No weight lies outside its bound. */
int gpd_hip_train_init_xavier(int channels, uint32_t seed, float *const tensors[8]);
/* Host only: the learning rate of update `it` (0-based) under the recipe's policy, the double result rounded to float once:
 * the definition the step uses.  GPD_ERR_INVALID: a null pointer, it < 0, a non-finite or negative base_lr, a policy the
 * recipe check above refuses. */
int gpd_hip_train_learning_rate(const gpd_train_recipe *recipe, double base_lr, long long it, float *lr);
/* The optimiser's buffers as eight tensors in state layout, and the update count.  Adam: m = exp_avg, v = exp_avg_sq; SGD:
 * m = the momentum history h, v is not touched and may be NULL.  gpd_hip_train_set_state clears all of it, so a resumed run is
 * set_state followed by set_solver_state: it then continues byte for byte.  GPD_ERR_INVALID (nothing changed): a NULL where
 * the solver has a buffer, a non-finite value, a negative count. */
/* gpd_hip_train_kernel_name for the launches of this trainer's timed step: the last one is "sgd" under solver 1. */
const char *gpd_hip_train_kernel_name_of(const gpd_hip_trainer *t, int i);
int gpd_hip_train_get_solver_state(gpd_hip_trainer *t, float *const m[8], float *const v[8], long long *count);
int gpd_hip_train_set_solver_state(gpd_hip_trainer *t, const float *const m[8], const float *const v[8], long long count);

/* ---- trainers of any network of the family (train.hip) ------------------------------------------------------
 * Everything above trains the stock widths (C, 20, 50, 500, 0).  gpd_hip_train_create_net trains any gpd_lenet_shape that
 * gpd_hip_lenet_shape_check accepts — pytorch/network.py::Net of other widths, and ::NetCCFFF with its third dense layer
 * (fc2_out = H2 > 0) — under either network variant (with or without the conv ReLUs) and either solver.  Data pools, steps,
 * eval, append_view, step_timed and the group take such a trainer as they take the stock one.
 *
 * The state of a trainer with H2 == 0 is the eight tensors above with sizes following its shape (F1 = conv1_out, F2 =
 * conv2_out, H1 = fc1_out): conv1.weight [F1][C][5][5], conv1.bias [F1], conv2.weight [F2][F1][5][5], conv2.bias [F2],
 * fc1.weight [H1][F2 * 144], fc1.bias [H1], fc2.weight [2][H1], fc2.bias [2]; the entries with tables of 8 serve it.  With
 * H2 > 0 there are ten: fc2.weight [H2][H1], fc2.bias [H2], fc3.weight [2][H2], fc3.bias [2]; the entries with tables of 8 then
 * return GPD_ERR_STATE and change nothing.  The gpd_hip_train_net_ entries take tables of 10 in the order of
 * gpd_hip_lenet_net_from_torch's input and serve every trainer; slots [8] and [9] are not read when H2 == 0 and may be NULL.
 *
 * Summation order (the stock shape's is unchanged): fc1 forward sums K = 144 F2 in 16 ranges of 9 F2; conv2's weight gradient
 * one partial per image, conv1's four per image, joined as before; the third dense layer is one chain per output forward
 * (K = H1), K = B for its weight gradient, K = H2 for the gradient it hands back, its bias and fc1's summed over the batch in
 * eight interleaved chains.  gpd_hip_train_step_timed lists four more launches for H2 > 0 (gpd_hip_train_kernel_name_of).
 *
 * gpd_hip_train_create_net: recipe may be NULL (gpd_hip_train_create's).  GPD_ERR_INVALID before anything is allocated, beyond
 * gpd_hip_train_create_recipe's: a NULL shape, a shape gpd_hip_lenet_shape_check refuses, shape->channels != params->channels,
 * H2 > 0 with any lr_mult or decay_mult other than 1 (the recipe has eight multiplier slots).  The stock shape through this
 * entry is gpd_hip_train_create_recipe byte for byte. */
int gpd_hip_train_create_net(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, const gpd_lenet_shape *shape,
                             gpd_hip_trainer **out);
int gpd_hip_train_shape(const gpd_hip_trainer *t, gpd_lenet_shape *out);
int gpd_hip_train_net_set_state(gpd_hip_trainer *t, const float *const tensors[10]);
int gpd_hip_train_net_get_state(gpd_hip_trainer *t, float *const tensors[10]);
int gpd_hip_train_net_gradients(gpd_hip_trainer *t, const int32_t *indices, int batch, float *const grads[10], float *loss);
int gpd_hip_train_net_apply(gpd_hip_trainer *t, const float *const grads[10]);
int gpd_hip_train_net_get_solver_state(gpd_hip_trainer *t, float *const m[10], float *const v[10], long long *count);
int gpd_hip_train_net_set_solver_state(gpd_hip_trainer *t, const float *const m[10], const float *const v[10], long long count);
/* Host only.  sizes: the element counts of the ten tensors (n[8] = n[9] = 0 when H2 == 0).  init_state / init_xavier:
 * gpd_hip_train_init_state / gpd_hip_train_init_xavier for the shape — the same stream, the tensors in order, fan_in 25 C,
 * 25 F1, 144 F2, H1, H2 — and their bytes at the stock shape.  GPD_ERR_INVALID, nothing written: a NULL argument, a NULL among
 * the used tensors, a shape outside the limits. */
int gpd_hip_train_net_sizes(const gpd_lenet_shape *shape, size_t n[10]);
int gpd_hip_train_net_init_state(const gpd_lenet_shape *shape, uint32_t seed, float *const tensors[10]);
int gpd_hip_train_net_init_xavier(const gpd_lenet_shape *shape, uint32_t seed, float *const tensors[10]);

/* ---- training on several replicas (train_group.hip, group_model.h) ---------------------------------------------
 * What pytorch/train_net3.py:97-99 gets from nn.DataParallel: G trainers ("replicas"), each on a context of its own — on G
 * devices, or several on one device — run forward and backward on a batch each, and every replica's solver applies the MEAN
 * of the G gradients.  The definition is the composed route — gpd_hip_train_gradients on every replica,
 * gpd_hip_train_group_mean on the host, gpd_hip_train_apply on every replica — and gpd_hip_train_group_steps is held to it
 * byte for byte while no parameter-sized buffer leaves the devices.
 *
 * Host only, the definition:
 *  - mean: per element s = g[0]; s = s + g[r] for r = 1 .. G - 1 in rank order; out = s * (float)(1.0 / G), every operation a
 *    rounded f32 operation, nothing fused.  G = 1: g[0]'s bits.  A step's loss is the same expression over the replicas' losses.
 *  - slices: [0, n) cut into G contiguous slices first[o] .. first[o + 1] (first holds G + 1 entries); every boundary but n is
 *    a multiple of 4 floats, the sizes differ by at most 4 floats.  Replica o sums slice o.
 *  - schedule: the list of operations gpd_hip_train_group_steps enqueues for num_steps steps, in the order in which it
 *    enqueues them from its one host thread (a stream's wait binds to the record enqueued last, so the order is part of the
 *    list's correctness).  An operation is five int32 {kind, stream, peer, slice, event}; stream = the replica on whose
 *    stream it goes; peer, slice, event are -1 where the kind has none.  kind 0: forward and backward of the replica's next
 *    batch; 1: wait on `event`; 2: record `event`; 3: copy slice `slice` of replica `peer`'s gradient buffer — slice ==
 *    stream: into the replica's gather row of `peer`, otherwise to the same place of its own gradient buffer; 4: the
 *    replica's own slice = the mean of its buffer and its gather rows, in place; 5: the solver's update.  Events: r = the
 *    gradients of replica r, G + o = the sum of owner o, 2 G + r = replica r holds every sum.  ops may be NULL (count only);
 *    *num = the operations of the list; GPD_ERR_CAPACITY if capacity is smaller.
 * GPD_ERR_INVALID: a null argument, G outside 1 .. 16, a negative count. */
int gpd_hip_train_group_mean(const float *const *g, int G, size_t n, float *out);
int gpd_hip_train_group_slices(size_t n, int G, long long *first);
int gpd_hip_train_group_schedule(int G, int num_steps, void *ops, int capacity, int *num);

typedef struct gpd_hip_train_group gpd_hip_train_group;
/* 1 <= num <= 16 trainers.  The group takes no ownership: it is destroyed before its trainers, and a trainer may still be
 * stepped alone (gpd_hip_train_group_verify then tells).  GPD_ERR_INVALID before anything is allocated: a null or repeated
 * trainer, two trainers on one context, channel counts, network widths, gpd_train_params (apart from max_batch) or recipes that
 * differ.
 * Allocates per replica a gather block of G - 1 slices and three events; never enables peer access. */
int gpd_hip_train_group_create(gpd_hip_trainer *const *trainers, int num, gpd_hip_train_group **out);
void gpd_hip_train_group_destroy(gpd_hip_train_group *g);
/* Replica src's parameters, solver buffers and update count into every other replica, device to device; returns after the
 * copies.  How a group starts (gpd_hip_train_set_state on one replica, then this) and how a snapshot resumes. */
int gpd_hip_train_group_broadcast(gpd_hip_train_group *g, int src);
/* num_steps updates.  In step s replica r runs forward and backward on the images indices[r][s * batch .. (s + 1) * batch) of
 * ITS OWN resident training set, the mean of the G gradients is formed on the devices (each replica sums one slice and hands
 * it round: 2 (G - 1) / G of a buffer moved per replica and step) and every replica's solver applies it: the replicas end
 * with identical bytes without a parameter broadcast.  losses [num_steps]: the mean of the replicas' losses by the same
 * expression; replica_losses (may be NULL) [num][num_steps].  The steps are enqueued back to back and waited for once (once per
 * 2^20 indices of a replica); no parameter-sized copy crosses to or from the host.  GPD_ERR_INVALID before anything is
 * launched, naming replica and position: a batch outside 1 .. max_batch of a replica, an index outside a replica's set. */
int gpd_hip_train_group_steps(gpd_hip_train_group *g, const int32_t *const *indices, int num_steps, int batch, float *losses,
                              float *replica_losses);
/* *num_different = the 32-bit words of the parameters and the solver buffers of replicas 1 .. num - 1 that differ from
 * replica 0's, counted on the devices (replica 0's buffers come over slice by slice), plus 1 for each replica whose update
 * count differs: 0 for a group that has only been stepped together since its broadcast. */
int gpd_hip_train_group_verify(gpd_hip_train_group *g, long long *num_different);
/* Bytes the last broadcast / steps / verify call moved: out[0] between replicas, out[1] between host and devices. */
int gpd_hip_train_group_last_bytes(gpd_hip_train_group *g, long long out[2]);

#ifdef __cplusplus
}
#endif
#endif /* GPD_HIP_H_ */
