/* shoulder_hip.h -- C-ABI of libshoulder_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the `shoulder.Humerus` landmark path of gregspangenberg/shoulder.
 * The reference has no FFI of its own (pure Python over NumPy/trimesh/onnxruntime); the
 * Python facade `shoulder_amd.Humerus` keeps the reference's accessor API and calls these
 * entry points through ctypes.  Each entry point names the reference code it replaces
 * (paths relative to src/shoulder/).
 *
 * Conventions: every function returns 0 (SH_OK) or a negative sh_status and never throws or
 * aborts across the boundary; sh_last_error() gives the text.  The caller owns every host
 * buffer; the library owns all device memory inside sh_ctx.  One sh_ctx per HIP device /
 * stream; a ctx is NOT thread-safe; distinct ctxs may run concurrently.  All work is
 * enqueued on the ctx's HIP stream; functions that return host data synchronise that stream.
 * Matrices are 4x4 row-major float64, points are xyz float64, vertices are float32 (as in
 * an STL file).
 */
#ifndef SHOULDER_HIP_H
#define SHOULDER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sh_ctx sh_ctx;

typedef enum sh_status {
  SH_OK = 0,
  SH_ERR_ARG = -1,      /* bad argument / shape */
  SH_ERR_HIP = -2,      /* HIP runtime error (text in sh_last_error) */
  SH_ERR_STATE = -3,    /* call order: meshes / parameters not loaded */
  SH_ERR_CAPACITY = -4, /* a capacity was exceeded.  Since round 5 the stages grow what they need (crossings and loops per
                           section, end-section points, hull vertices / faces, silhouette edges of a box candidate: the run
                           is repeated inside sh_collect) -- what is left: a caller-sized output that is too small (the
                           counts returned say how large), more than 1 024 closed loops in ONE section, and a growth
                           that is needed while a second run is in flight (collect it, run again) */
  SH_ERR_GEOMETRY = -5, /* degenerate input: open contour (SH_OPEN_ERROR mode; see sh_set_open_contours), empty slice, ray miss, ... */
  SH_ERR_NOMEM = -6,
  SH_ERR_INTERNAL = -8  /* an invariant of the library did not hold (sh_geodesic: a relaxation went past the rounds its rule allows) */
} sh_status;

/* Stages of sh_run, in evaluation order (bone.py:110-157). */
enum {
  SH_STAGE_OBB      = 1u << 0, /* mesh.py:63-125  FullObb._obb (hull, min-volume box, head-end flip) */
  SH_STAGE_FULL     = 1u << 1, /* slice.py:209-224 + :21-60  FullSlices sections, centroids, areas   */
  SH_STAGE_NECK     = 1u << 2, /* surgical_neck.py:22-56  kernel change point -> neck_z              */
  SH_STAGE_CANAL    = 1u << 3, /* canal.py:19-85                                                     */
  SH_STAGE_PROXIMAL = 1u << 4, /* slice.py:227-253 + :65-147 ProximalSlices, resample, polar images  */
  SH_STAGE_GROOVE   = 1u << 5, /* bicipital_groove.py:26-265                                         */
  SH_STAGE_ANP      = 1u << 6, /* anatomic_neck.py:31-236 (image, UNet, edge points, plane, axes)    */
  SH_STAGE_DISTAL   = 1u << 7, /* slice.py:256-276 DistalSlices sections                             */
  SH_STAGE_TE       = 1u << 8, /* epicondyle.py:29-101                                               */
  SH_STAGE_CSYS     = 1u << 9, /* bone.py:146-157 construct_csys + re-expression of landmarks        */
  SH_STAGE_APPLY    = 1u << 10,/* bone.py:155 `mesh_ct.copy().apply_transform(csys)` for the whole batch: device buffer
                                  "verts_csys" (sumV x 3 float64) = csys[b] * vertices of mesh b; needs SH_STAGE_CSYS in
                                  the same run                                                        */
  SH_STAGE_ALL      = 0x7FFu
};

/* Arithmetic of the anatomic-neck network (the ONNX session of anatomic_neck.py:62-76 computes in float32):
 * F32  one float32 fma chain per output on v_mfma_f32_16x16x4_f32 -- bit-exact against oracle/unet_chain.c;
 * BF16 / F16  16-bit activations and weights on v_mfma_f32_16x16x32_{bf16,f16}, float32 accumulate (throughput paths;
 *      F16 carries 11 significant bits instead of 8 and needs activations below 65504). */
enum { SH_UNET_F32 = 0, SH_UNET_BF16 = 1, SH_UNET_F16 = 2,
       SH_UNET_F32X = 3 };      /* f32 tensors, MFMA layers on split f16 operands (3 MFMAs per product): f32-grade logits at ~5x the f32 rate.
                                 * Range (the operands are pairs of f16 values): weights of the >= 32-channel layers need |w| < 1023.5
                                 * (= 65504 / 64; a run with a larger weight returns SH_ERR_ARG and names the layer), activations need
                                 * |x| < 65504 (beyond it an operand's high part is an infinity and the logits NaN, as in F16), and the
                                 * low part of an activation below 2^-14 falls into f16's subnormals (absolute error <= 2^-25).  The
                                 * reference's input is an image in [0, 1] (anatomic_neck.py:57); SH_UNET_F32 has none of these limits. */
/* Which facade class of bone.py the meshes are: `Humerus` (bone.py:110-157) or `ProximalHumerus` (bone.py:24-64: a
 * humerus cut in the shaft -- ProxObb head-end rule and canal range mesh.py:128-192, neck cut-off (0.2, 0.99)
 * surgical_neck.py:25-26, canal cut-offs from the box canal.py:33-38, no distal / trans-epicondylar stage,
 * csys = apply_csys_canal_articular bone.py:53-62). */
enum { SH_BONE_HUMERUS = 0, SH_BONE_PROXIMAL = 1 };

#define SH_GROOVE_ROWS 330   /* rows 150..479 of 600 proximal slices (slice.py:157-164) */
#define SH_ANP_MAX_PTS 4096  /* capacity of the padded edge-point list                  */

/* Fixed-size result per humerus; everything in CT coordinates unless noted.
 * Row order of every (2,3) axis follows the reference accessor it mirrors. */
typedef struct sh_landmarks {
  double obb_transform[16];   /* FullObb.transform, CT -> OBB incl. head-end flip (mesh.py:124) */
  double z_length;            /* mesh.py:86 */
  double neck_z;              /* SurgicalNeck.neck_z, OBB frame (surgical_neck.py:34) */
  double canal_axis[6];       /* Canal.axis(): [proximal, distal] (canal.py:58-85) */
  double te_axis[6];          /* TransEpicondylar.axis(): [medial, lateral] (epicondyle.py:29-101) */
  double groove_axis[6];      /* DeepGroove.axis() (bicipital_groove.py:244-265) */
  double bg_theta;            /* DeepGroove.bg_theta (bicipital_groove.py:188) */
  double anp_plane_point[3];  /* AnatomicNeck.plane().point  (anatomic_neck.py:123-153) */
  double anp_plane_normal[3]; /* AnatomicNeck.plane().normal */
  double anp_axis_normal[6];  /* AnatomicNeck.axis_normal(): [upper, lower] (anatomic_neck.py:174-200) */
  double anp_axis_central[6]; /* AnatomicNeck.axis_central(): [upper, lower] (anatomic_neck.py:202-236) */
  double csys[16];            /* apply_csys_canal_transepiconylar() matrix, CT -> canal/TE (bone.py:146-157);
                                 SH_BONE_PROXIMAL: apply_csys_canal_articular() (bone.py:53-62) */
  double csys_articular[16];  /* apply_csys_canal_articular() matrix, CT -> canal / head-normal axis (bone.py:53-62), both bone kinds */
  double neckshaft;           /* NeckShaft.calc(), degrees (bone_props.py:88-112) */
  double retroversion;        /* RetroVersion.calc() with landmarks in CT, degrees (bone_props.py:50-85); NaN for SH_BONE_PROXIMAL */
  double radius_curvature;    /* RadiusCurvature.calc(), mm (bone_props.py:115-148) */
  double canal_cutoff[2];     /* cut-off fractions the canal used: sh_params.canal_cutoff, or ProxObb.cutoff_pcts (mesh.py:190) */
  double groove_points[SH_GROOVE_ROWS * 3]; /* DeepGroove.points() (bicipital_groove.py:26-242) */
  double anp_points[SH_ANP_MAX_PTS * 3];    /* AnatomicNeck.points(), first n_anp rows valid (anatomic_neck.py:31-121) */
  int32_t n_anp;              /* number of edge points (K) */
  int32_t n_articular;        /* number of mask pixels (anatomic_neck.py:104-112) */
  int32_t neck_index;         /* change-point index into areas1((0.70,0.99)) (surgical_neck.py:33) */
  int32_t flipped;            /* 1 if the head end was at -z of the raw box (mesh.py:112) */
  int32_t status;             /* 0 or a negative sh_status for this mesh */
  int32_t side;               /* Side.calc(): 0 = "left", 1 = "right" (bone_props.py:12-47) */
} sh_landmarks;

/* Tunables the reference exposes as keyword defaults (SURVEY 5 "config / flags"). */
typedef struct sh_params {
  double canal_cutoff[2];     /* canal.py:19          default (0.35, 0.75) */
  double groove_cutoff[2];    /* bicipital_groove.py:26 default (0.2, 0.75); rows must stay 330 */
  double groove_deg_window;   /* bicipital_groove.py:26 default 7 */
  int32_t unet_dtype;         /* SH_UNET_F32 (parity), SH_UNET_F32X (f32-grade, fast), SH_UNET_BF16 or SH_UNET_F16 (throughput) */
  int32_t bone_kind;          /* SH_BONE_HUMERUS (default) or SH_BONE_PROXIMAL */
} sh_params;

/* ---- context ------------------------------------------------------------------------ */
int  sh_ctx_create(int device, void* hip_stream /* nullable: e.g. torch's current stream */, sh_ctx** out);
void sh_ctx_destroy(sh_ctx*);
const char* sh_last_error(const sh_ctx*);      /* owned by ctx, valid until the next call */
int  sh_default_params(sh_params* out);
int  sh_set_params(sh_ctx*, const sh_params*);
int  sh_get_params(const sh_ctx*, sh_params* out);   /* the values in force (read-modify-write with sh_set_params) */

/* ---- parameters (replace the ONNX files read at bicipital_groove.py:174-180 and
 *      anatomic_neck.py:62-69; host pointers, copied) ---------------------------------- */
int  sh_load_rfc(sh_ctx*, const int32_t* feat, const float* thr, const int32_t* true_idx,
                 const int32_t* false_idx, const float* leaf_weight, int n_nodes,
                 const int32_t* roots, int n_trees);
/* UNet: `packed` = concatenation, in this order, of enc{i}a_w,enc{i}a_b,enc{i}b_w,enc{i}b_b (i=0..depth-1),
 * bota_w,bota_b,botb_w,botb_b, then for i=depth-1..0: up{i}_w,up{i}_b,dec{i}a_w,dec{i}a_b,dec{i}b_w,dec{i}b_b,
 * then head_w, head_b; conv weights laid out [ky][kx][cin][cout] float32 (csrc/sh_unet_plan.h unet_layers_in_block_order
 * states the order and the shapes).  base_channels: a multiple of 32, at most 256; depth 1..6. */
int  sh_load_unet(sh_ctx*, int base_channels, int depth, const float* packed, size_t n_floats);
/* Device address + size of the packed parameter block, for a collective broadcast by the caller (torch.distributed over
 * RCCL); valid until the next sh_load_*.  The block is `packed` as sh_load_unet took it, then the arrays of sh_load_rfc in
 * the order of its arguments (n_nodes elements each, roots n_trees), 4-byte elements, nothing between them:
 * csrc/sh_params.h (SH_PARAM_SECTIONS) is the statement of this layout. */
int  sh_param_block(sh_ctx*, void** dev_ptr, size_t* nbytes);
/* After the caller has overwritten the device parameter block (the receiving ranks of a broadcast): re-read the host
 * mirrors from it, so that a later sh_load_rfc / sh_load_unet -- which re-uploads the whole block from the mirrors --
 * does not put stale values back.  The forest's topology (child indices, roots) is validated like in sh_load_rfc. */
int  sh_param_block_commit(sh_ctx*);
/* (The 16-bit UNet paths pack their weights from this block once and keep the packed copy until the block can have
 * changed: sh_load_*, sh_param_block / sh_buffer_device("params") handing the pointer out, sh_param_block_commit, sh_store.
 * A caller that keeps the pointer and writes the block again later must call sh_param_block_commit again.) */

/* ---- meshes (replace MeshLoader, mesh.py:14-41; vertices already merged) ------------- */
int  sh_upload_meshes(sh_ctx*, const float* verts /* sumV x 3 */, const int32_t* faces /* sumF x 3, per-mesh local ids */,
                      const int64_t* v_off /* B+1 */, const int64_t* f_off /* B+1 */, int B);
/* The same from B binary STL files held in host memory (`trimesh.load_mesh(stl_file)` at mesh.py:22-27 incl. its vertex
 * merge): records are parsed and merged on the device -- vertices with equal bit patterns (after -0.0 -> +0.0) become
 * one, numbered by first appearance in the file; triangles that use a vertex twice are dropped.  v_off_out / f_off_out
 * (B+1 each, nullable) receive the resulting offsets. */
int  sh_upload_stl(sh_ctx*, const void* const* files, const size_t* nbytes, int B, int64_t* v_off_out, int64_t* f_off_out);
/* A stream of NEW batches (the reference's unit of work is a new STL: mesh.py:22-27, bone.py:110-131).  sh_upload_* hands a
 * batch over synchronously; the staging calls hand the NEXT batch over while a run of the resident one executes:
 *   sh_stage_meshes / sh_stage_stl  same arguments and checks as sh_upload_meshes / sh_upload_stl.  The call checks sizes and
 *     headers and returns at once; a background thread copies the arrays / files through page-locked staging (page-locked
 *     caller memory -- sh_host_alloc -- is read in place) into buffers of their own on a copy stream, element checks and the STL
 *     parse / vertex merge run on the device, and the convex hulls of the staged batch (host hull mode) are computed by the same
 *     thread.  THE CALLER KEEPS THE ARRAYS / FILES UNCHANGED UNTIL sh_commit_staged HAS RETURNED (or the batch is replaced: staging
 *     again, any sh_upload_* / sh_synth_batch).  One batch can be staged at a time.
 *   sh_commit_staged  makes the staged batch the resident one (buffer entries are swapped, nothing is copied).  Needs the context
 *     idle (sh_collect every run first).  Reports what sh_upload_* would have reported for a bad batch (SH_ERR_ARG; the resident
 *     batch stays).  The next sh_submit / sh_run finds the hulls prepared.  v_off_out / f_off_out (B+1 each, nullable): offsets.
 * A run submitted between stage and commit belongs to the resident batch and voids the staged batch's prepared hulls (they are
 * computed again by its first run).  Keep sh_set_overlap off on a context that streams: a batch that runs once needs no hulls
 * prepared for a second run, and the staging call would wait for that preparation.  Records are identical to sh_upload_*
 * followed by the same runs. */
int  sh_stage_meshes(sh_ctx*, const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int B);
int  sh_stage_stl(sh_ctx*, const void* const* files, const size_t* nbytes, int B);
int  sh_commit_staged(sh_ctx*, int64_t* v_off_out, int64_t* f_off_out);
int  sh_staged(const sh_ctx*);      /* 1 while a staged batch waits for its commit */
/* Synthetic batch (BASELINE config 3/4): mesh i = similarity transform T[i] (4x4, float64)
 * of uploaded mesh 0, evaluated on the device in float64 and stored as float32. */
int  sh_synth_batch(sh_ctx*, const double* T /* B x 16 */, int B);
int  sh_batch_size(const sh_ctx*);

/* The proximal slice set's resampling (slice.py:65-147, 166-206) makes three arrays per plane -- the 512-sample contour ("prox.ixy")
 * and its polar rows about the origin / about the centroid ("prox.itr_start" / "prox.itr_centered_start") -- 24 KB per plane, 944 MB
 * per batch of 64.  The stages behind read part of them only (polar rows about the origin from plane 88 on: anatomic_neck.py:34;
 * centred rows inside the groove's cut-off range: bicipital_groove.py:63-67; the contour never), and that is what a run writes.
 * sh_set_keep_products(ctx, 1): every plane's three arrays are written (for sh_fetch: the reference keeps them as
 * `Slices.ixy / itr_start / itr_centered_start`).  A run of SH_STAGE_GROOVE without SH_STAGE_PROXIMAL after groove_cutoff changed
 * returns SH_ERR_STATE: the rows it needs were not written. */
int  sh_set_keep_products(sh_ctx*, int on);

/* Meshes that are not watertight.  The reference warns and carries on (humerus/mesh.py:24-27 `if not mesh.is_watertight:
 * warnings.warn(...)`) and resamples `slice.discrete[0]` whether that path is closed or not (slice.py:65-80).
 * SH_OPEN_ERROR (the default): a section with an open chain of crossing segments is SH_ERR_GEOMETRY for that humerus.
 * SH_OPEN_BRIDGE: in every plane of every slice set (slice.py:21-60 full / distal / proximal sets, surgical_neck.py:37-39 neck
 * contour, mesh.py:157-160 ProxObb area scan) a chain's tail t is joined to a chain's head h by a virtual segment when the gap
 * |end(t) - start(h)| <= max_gap (mm, box-frame xy), smallest (gap, end key of t, start key of h) first; the bridge adds one
 * ring vertex, the crossing on t's end edge.  Loops are the cycles of three or more vertices; segments on no loop are dropped
 * (max_gap = 0: oracle/section.py's "drop open chains").  A plane left without a loop is SH_ERR_GEOMETRY as before (an empty
 * area-scan section stays legal).  A single missing triangle is bridged by its own segment: the intact mesh's records.
 * max_gap: finite and >= 0, else SH_ERR_ARG; default SH_OPEN_GAP_DEFAULT (the longest edge of the test meshes, 11.46 mm, rounded
 * up).  Not while runs are in flight (SH_ERR_STATE).  Multi-hit rays, non-manifold edges and sh_clip's open contours stay errors. */
enum { SH_OPEN_ERROR = 0, SH_OPEN_BRIDGE = 1 };
#define SH_OPEN_GAP_DEFAULT 12.0
int  sh_set_open_contours(sh_ctx*, int mode, double max_gap);
int  sh_get_open_contours(const sh_ctx*, int* mode, double* max_gap);
/* Per humerus of the last run: open chains closed by bridges and open chains dropped (bridged + dropped = the chains of every
 * section; 0 / 0 after a run in SH_OPEN_ERROR mode).  bridged, dropped: B int32 each. */
int  sh_open_contour_stats(sh_ctx*, int32_t* bridged /* B */, int32_t* dropped /* B */);
/* `not mesh.is_watertight` (humerus/mesh.py:24) as a count: per resident mesh, the undirected edges used by a number of faces
 * other than two (0: every edge has two faces).  On demand, outside sh_run.  out: B int64. */
int  sh_mesh_open_edges(sh_ctx*, int64_t* out /* B */);

/* Records on the wire.  A full sh_landmarks record is 104 KB, 96 KB of it the padded anatomic-neck point list (4 096 rows; a
 * humerus has about a thousand).  sh_set_record_rows(R), R > 0: every record a run hands out through `out` of sh_run /
 * sh_submit (host memory or a gather's device send buffer) is PACKED to sh_record_bytes(R) = 8 680 + 24 R bytes:
 *   [the bytes of sh_landmarks in front of anp_points] [its six trailing int32 fields: n_anp, n_articular, neck_index,
 *   flipped, status, side] [R rows of anp_points: the first min(n_anp, R), zeros behind them]
 * n_anp keeps the true count; sh_anp_points returns every point of one humerus of the last run (CT, the record's own
 * arithmetic) whatever the format.  R = 0 (default): full records.  The device records (sh_landmarks_device) are always full. */
int  sh_set_record_rows(sh_ctx*, int anp_rows);
size_t sh_record_bytes(int anp_rows);
int  sh_anp_points(sh_ctx*, int b, double* out /* cap x 3 */, int cap, int* n_out);

/* ---- the hot path -------------------------------------------------------------------- */
int  sh_run(sh_ctx*, uint32_t stage_mask, sh_landmarks* out /* B, host, nullable */);
/* The same in two halves, for callers that stream runs: sh_submit enqueues a run (all device work, the copy of the records to
 * `out` -- page-locked memory, see sh_host_alloc, or the call blocks -- and of the per-mesh status words) and returns;
 * sh_collect waits for the oldest submitted run and reports its status like sh_run.  At most two runs may be in flight, so
 * the device goes from one run to the next without waiting for the host.  sh_run = sh_submit + sh_collect. */
int  sh_submit(sh_ctx*, uint32_t stage_mask, sh_landmarks* out /* B, host, nullable */);
int  sh_collect(sh_ctx*);
/* Device address of the B result structs of the last sh_run (for a collective gather). */
int  sh_landmarks_device(sh_ctx*, void** dev_ptr, size_t* nbytes);
/* ---- several GPUs from ONE host process (a host in C, C++ or any FFI that does not launch one process per GPU) ----
 * One sh_ctx per device; the humeri of a cohort are sharded over the contexts (independent units of work: the reference runs one
 * `Humerus(stl)` at a time, bone.py:110-131), each context runs its shard (sh_submit on every context, then sh_collect), and
 * the records come together at ctxs[0].  What crosses the xGMI links: the parameter block once (the reference loads the same
 * pickled forest / ONNX blob in every process: bicipital_groove.py:21-25, anatomic_neck.py:56-60) and the records once per step
 * -- no exchange inside the path.  RCCL is loaded at run time by sh_comm_init_all (librccl.so.1, or the path in SHOULDER_RCCL_LIB);
 * nothing else in the library needs it.  Errors of these three calls are left on ctxs[0] (sh_last_error).  The multi-process
 * launch (bench.py --gpus N, one rank per GPU under torch.distributed) does the same transfers in shoulder_amd/dist.py.
 *   sh_comm_init_all     ncclCommInitAll over the contexts' devices (distinct devices); rank i = ctxs[i].  A context leaves its group
 *                        when it is destroyed or put into another.
 *   sh_bcast_weights     the parameter block of ctxs[root] (layout of sh_param_block) to every context; each has loaded a network
 *                        and a forest of the same shape before (any values); receivers validate the block like sh_param_block_commit.
 *   sh_gather_landmarks  the records of every context's last run, rank order, to host memory at ctxs[0]: sum of the batch sizes
 *                        records of sh_record_bytes(rows) bytes each, `rows` = the record format all contexts are set to
 *                        (sh_set_record_rows; 0 = full sh_landmarks).
 * STATUS: EXPERIMENTAL for n > 1.  The build pool has one GPU per box: these calls have run on hardware as a group of ONE only
 * (tests/test_gpu_comm.py prints the world size it ran with); the n > 1 legs -- the multi-rank ncclBroadcast, the grouped
 * ncclSend / ncclRecv of the gather, destroying one rank's communicator while its siblings live -- are untested on hardware. */
int  sh_comm_init_all(sh_ctx** ctxs, int n);
int  sh_bcast_weights(sh_ctx** ctxs, int n, int root);
int  sh_gather_landmarks(sh_ctx** ctxs, int n, sh_landmarks* out_root /* host */);
/* Page-locked host memory for the `out` array of sh_run when it is reused from run to run (the reference returns fresh
 * NumPy arrays from every accessor; a streaming caller keeps one record buffer): direct D2H, no page faults. */
int  sh_host_alloc(sh_ctx*, size_t nbytes, void** out);
int  sh_host_free(sh_ctx*, void* p);

/* utils.transform_pts (utils.py:172-188) for B point sets on the device:
 * out[off[b]..off[b+1]) = T[b] * in[...]; in/out are DEVICE pointers to float64 xyz. */
int  sh_affine_apply(sh_ctx*, const double* T /* host, B x 16 */, const void* dev_in, void* dev_out,
                     const int64_t* off /* host, B+1 */, int B);
/* Trimesh.apply_transform of mesh b (bone.py:155): transformed float64 vertices -> host. */
int  sh_mesh_transformed(sh_ctx*, int b, const double* T /* 16 */, double* out_verts /* V x 3 */);
/* utils.transform_pts for one host point set (every Landmark.transform_landmark, e.g. canal.py:84,
 * anatomic_neck.py:120): upload n xyz float64, transform on the device, download. */
int  sh_transform_points(sh_ctx*, const double* T /* 16 */, const double* in_pts /* host, n x 3 */, int n, double* out_pts /* host */);

/* The closed largest loop of plane k of slice set `set` ("distal", "prox", "neckc") of humerus b after a run -- what
 * `Slices.slices[k].polygons_closed[...]` exterior holds in the reference (slice.py:53-59, surgical_neck.py:37-54): n + 1
 * points (x, y) in the box frame, counter-clockwise, canonical start (rule B-1), first = last.  Read from the fixed slot range
 * or, for a plane with more crossing segments than slots, from the overflow pool.  out == NULL or cap < n + 1: only
 * *n_out = n + 1 is set. */
int  sh_ring(sh_ctx*, const char* set, int b, int k, double* out, int cap, int* n_out);
/* `mesh_ct.section(plane_origin, plane_normal).vertices` for mesh b (AnatomicNeck.plane_points,
 * anatomic_neck.py:155-172): unique crossing points of one general plane, CT coordinates, unordered. */
int  sh_section_plane(sh_ctx*, int b, const double* origin /* 3 */, const double* normal /* 3 */, double* out_pts /* cap x 3 */,
                      int cap, int* n_out);

/* `mesh.slice_plane(origin, normal)` (HumeralHeadOsteotomy.resect_mesh, arthroplasty.py:80-87; trimesh
 * slice_faces_plane + the constructor's 8-decimal vertex merge) for ONE mesh given as host arrays in any coordinate
 * system and P planes at once (a sweep of resection planes is one call): per plane the part on the side the normal
 * points to -- kept faces, cut faces re-triangulated, unreferenced vertices dropped, vertices merged.  Vertex order is
 * this library's canonical one (by first use; trimesh's depends on its hash sort), faces keep trimesh's order.
 * out_edges (nullable): per cut face the edge between its two new vertices = the section polyline of the plane
 * (HumeralHeadOsteotomy.points, arthroplasty.py:69-78).  counts: P x (n_verts, n_faces, n_edges).
 * out_verts == NULL: count only; counts then hold capacities that suffice (n_verts is an upper bound). */
int  sh_slice_mesh_planes(sh_ctx*, const double* verts /* nv x 3 */, int nv, const int32_t* faces /* nf x 3 */, int nf,
                          const double* origins /* P x 3 */, const double* normals /* P x 3 */, int P,
                          double* out_verts /* P x cap_v x 3 */, int cap_v, int32_t* out_faces /* P x cap_f x 3 */, int cap_f,
                          int32_t* out_edges /* P x cap_e x 2 */, int cap_e, int32_t* counts /* P x 3 */);

/* ---- batched head resection: B resident humeri x P planes in one device pass ----------------------------------------
 * `HumeralHeadOsteotomy` (arthroplasty.py:13-175) for a cohort: what a planning sweep reads off a cut -- the cut contour, its
 * area, the volume and height of the resected head -- as one fixed-size record per (humerus, plane), from the vertices and
 * faces that are resident on the device (nothing is uploaded again, no mesh comes back).  The mesh of a humerus is read once
 * for all of its P planes (k_resect.h).  Records and rings are reproducible bit for bit and do not depend on the batch a
 * humerus is measured in, its position there or P (per-tile partial sums stored and added in a fixed order, no float atomics).
 *
 * Cut semantics are sh_slice_mesh_planes' (`Trimesh.slice_plane`, arthroplasty.py:80-87; oracle/clip.py): sign of a vertex
 * with tolerance 1e-8 on dot(v - point, normal) -- the normal is used AS GIVEN, not rescaled, like trimesh does -- class of a
 * face from its three signs, crossing point a + (num / den) d per face edge, faces lying in the plane decided by their own
 * normal.  The section is joined on mesh-edge keys (a crossing that is a mesh vertex, |dot| <= 1e-8: on that vertex' id); of two
 * faces that compute the crossing of one edge the one `slice_plane`'s vertex merge keeps is taken.  Meshes are taken to be
 * consistently oriented, as everywhere in the slice layer.
 *   status SH_ERR_GEOMETRY  a section with an open chain / a vertex used by other than two segments (`points()` would not get
 *                           closed loops from it); the face sums (head_*, n_cut_faces) stay valid, ring fields are zero.  Resection
 *                           contours are not bridged (sh_set_open_contours does not apply here).
 *   status SH_ERR_CAPACITY  a section with more than 1 024 crossing segments (SH_MAXSEG) or more than 32 loops: NOT joined through
 *                           the overflow pool; the face sums stay valid, ring fields are zero.  Never a wrong ring, never a failed batch. */
typedef struct sh_cut_offset {          /* one planned cut relative to a humerus' native anatomic-neck plane; applied in this order: */
  double retroversion_deg;              /* HumeralHeadOsteotomy.offset_retroversion   (arthroplasty.py:90-104)   */
  double neckshaft_deg;                 /* .offest_neckshaft                          (:106-118)                 */
  double depth_canal_mm, depth_anp_mm, depth_resection_mm;   /* .offset_depth(mm, "canal" / "anp" / "resection") (:120-145) */
  double anterior_mm;                   /* .offset_anterior_posterior                 (:147-162)                 */
  double medial_mm;                     /* .offset_medial_lateral                     (:164-175)                 */
} sh_cut_offset;                        /* a field that is exactly 0 is a call that is not made: all zeros = the native plane (into the csys and back) */

typedef struct sh_resection {           /* one (humerus, plane); CT coordinates */
  double plane_point[3], plane_normal[3];  /* the plane that was cut; the normal as it was cut with (sh_resect_offsets: unit up to
                                              rounding, sh_resect_planes: the caller's) -- feeding them back gives the same record */
  double head_volume;    /* mm^3: sum over the faces of the normal's side, cut faces re-triangulated as slice_plane does, of
                            det(a-o, b-o, c-o)/6 about o = plane_point -- the flat cap contributes nothing about o */
  double head_area;      /* mm^2: area of those faces (no cap) */
  double head_height;    /* mm: largest distance dot(v - o, n) / |n| of a vertex of a face from the plane on the normal's side; 0 if none */
  double cut_area, cut_perimeter, cut_centroid[3];  /* of the LARGEST loop (= points(), arthroplasty.py:69-78): |shoelace area| in
                            base.Section's in-plane basis (u = n x e_x, or n x e_y when |n_x| >= 0.9, normalised; w = n x u) with
                            coordinates taken about o; length of the closed ring; area centroid of the polygon */
  double cap_area;       /* |sum of the signed areas of all loops| (outer loops minus holes) */
  int32_t n_loops, n_ring, n_cut_faces, status;     /* loops; vertices of the largest (open count); faces the plane cuts;
                                                       0 or a negative sh_status for this cut */
} sh_resection;

/* P explicit planes per humerus.  Needs a resident batch only (no run).  P in 1..4096; a zero or non-finite normal or a
 * non-finite point: SH_ERR_ARG.  Not while runs are in flight (SH_ERR_STATE).  One device-to-host copy of the B x P records. */
int sh_resect_planes (sh_ctx*, const double* planes /* B x P x (point, normal), CT */, int P, sh_resection* out /* B x P, host */);
/* The same P offsets for every humerus; the plane of cut p of humerus b is built ON THE DEVICE from b's record of the last run
 * (anp_plane_*, csys_articular, side): what a fresh HumeralHeadOsteotomy of that humerus gives after the calls named in
 * sh_cut_offset, in that order, mapped back to CT (sh_scalar.h resect_plane_from_offsets; oracle/osteotomy.py).  Needs a
 * collected run of the resident batch that included SH_STAGE_ANP and SH_STAGE_CSYS (SH_ERR_STATE otherwise).  A humerus whose
 * record has status != 0 gets that status in all of its cuts (other fields zero); the batch does not fail.  Both bone kinds. */
int sh_resect_offsets(sh_ctx*, const sh_cut_offset* offs /* P, the same for every humerus */, int P, sh_resection* out /* B x P, host */);
/* The largest loop of cut p of humerus b of the last sh_resect_*: n_ring + 1 points, CT, closed (first = last), counter-clockwise
 * seen from the tip of the normal, starting at the crossing on the mesh edge with the smallest (min vid, max vid) key (rule B-1).
 * The cut is joined again for the call (the batch's rings are not kept: 24 KB per cut).  out == NULL or cap < n + 1: only
 * *n_out = n + 1 is set; a cut without a ring (status != 0, no loop): *n_out = 0. */
int sh_resect_ring   (sh_ctx*, int b, int p, double* out /* cap x 3, CT */, int cap, int* n_out);

/* ---- head sizing of a cut: the spherical cap that replaces the resected head and the ellipse of the cut it sits on --------
 * The reference stops in front of this step (arthroplasty.py:178-182, a commented-out `HumeralImplantation`); its
 * `RadiusCurvature` (bone_props.py:114-148) fits one sphere to the articular points of the NATIVE head.  Here every cut of a
 * batched resection gets the sphere of ITS head piece and the two diameters of ITS cut, in the same device pass (k_headfit.h).
 *
 * For a cut (o = plane_point, n = plane_normal) let T be the triangles whose terms enter head_volume / head_area: whole faces
 * on the normal's side, the two triangles (a, b, n0), (n0, n1, a) of a cut quad, the one triangle of a cut corner, as
 * `slice_plane` re-triangulates them (oracle/clip.py).
 *   samples   every corner p of every triangle of T, weight w = A / 3 (A the triangle's area: the surface lumped onto its
 *             vertices, so the fit does not follow mesh density), coordinates q = p - o (the terms stay small, as head_volume's)
 *   moments   sixteen doubles per cut: S0 = sum w | S1 = sum w q (3) | S2 = sum w q q^T (xx, xy, xz, yy, yz, zz) | S3 = sum w |q|^2 q
 *             (3) | S4 = sum w |q|^4 | two zero words.  Per (humerus, plane, tile of 256 faces) they are reduced in a fixed order
 *             and stored, the tiles are added in tile order: the moments, and with them the whole record, are the same bits
 *             whatever the batch, the humerus' position in it or P.  Named buffer "resect.fit_moments" (B x P x 16 doubles, sh_fetch).
 *   sphere    weighted algebraic least squares: minimise sum w (|q|^2 - 2 c.q - t)^2, normal equations
 *             [[4 S2, 2 S1], [2 S1^T, S0]] [c; t] = [2 S3; tr S2], r = sqrt(t + |c|^2), centre o + c; solved after a shift to the
 *             weighted centroid (sh_scalar.h head_sphere_from_moments, the same source on host and device).
 *             sphere_rms = sqrt(max(E, 0) / S0) / (2 r), E = S4 - rhs.[c; t] the minimum of the objective: the radial rms to
 *             first order, mm.  cap_height = r + c.n / |n|: thickness of the sphere's cap above the plane.
 *   ellipse   of the LARGEST loop (the one cut_area / cut_centroid describe): the polygon's area second moments about its area
 *             centroid in base.Section's basis (u, w) (see sh_resection), divided by the polygon area, eigenvalues l1 >= l2;
 *             cut_semi_major = 2 sqrt(l1), cut_semi_minor = 2 sqrt(l2): the semi-axes of the ellipse with the same area moments.
 *             cut_major_dir: unit eigenvector of l1 in CT, its first non-zero component (x, y, z order) positive.
 *   offsets   center_articular = csys_articular of the humerus' record applied to the sphere centre: origin at the canal-axis
 *             midpoint, z the canal, so x / y are the posterior-anterior / lateral-medial offsets in the conventions of
 *             sh_cut_offset's anterior_mm / medial_mm.  NaN when the resident batch has no collected run with SH_STAGE_ANP |
 *             SH_STAGE_CSYS (possible with sh_resect_planes_fit) or the humerus' record failed.
 * sphere_status: 0 with all sphere fields 0 for an empty piece (S0 = 0); SH_ERR_GEOMETRY with sphere fields 0 when the normal
 * matrix is not safely positive definite (all samples coplanar, ...: pivot threshold in sh_scalar.h).  ring_status: the cut's
 * own status (sh_resection.status); ring fields are zero when it is non-zero or the cut has no loop.  A humerus whose record
 * failed (sh_resect_offsets_fit) carries that status in both.  A bad fit never fails the batch. */
typedef struct sh_head_fit {
  double sphere_center[3], sphere_radius, sphere_rms, cap_height, fit_area /* = S0 */;
  double center_articular[3];
  double cut_semi_major, cut_semi_minor, cut_major_dir[3];
  int32_t sphere_status, ring_status;   /* 0 or a negative sh_status, each for its half */
} sh_head_fit;
/* sh_resect_planes / sh_resect_offsets with the head fit of every cut: same preconditions, argument checks and state errors;
 * `out` is byte-equal to what the un-fitted call writes for the same cuts (the same kernels write it); fit_out: B x P, host.
 * A sweep is split into passes of at most 4 096 cuts (the un-fitted calls: 8 192) and 128 MB of moment slab (128 B per cut
 * and tile); the pass a cut falls into does not change its records. */
int sh_resect_planes_fit (sh_ctx*, const double* planes, int P, sh_resection* out, sh_head_fit* fit_out);
int sh_resect_offsets_fit(sh_ctx*, const sh_cut_offset* offs, int P, sh_resection* out, sh_head_fit* fit_out);

/* ---- seating a catalogue of implant heads on every cut -----------------------------------------------------------------------
 * How each head of a catalogue sits on each cut of a fitted resection, computed on the device in the same pass (k_seat.h): the
 * ring of a cut never goes to the host.
 *
 * An implant head k is (R_k, h_k): radius of curvature and thickness, valid for 0 < h_k < 2 R_k.  Its base is a disk of radius
 * rho_k = sqrt(h_k (2 R_k - h_k)).  Geometry is taken in the cut's in-plane basis (u, w) of base.Section about o = plane_point,
 * exactly as cut_area / cut_centroid are (see sh_resection); the polygon is the LARGEST loop, the one cut_area describes, in
 * sh_resect_ring's order (counter-clockwise seen from the tip of the normal, canonical start); n^ = n / |n|.
 *   seat centre s   SH_SEAT_CUT_CENTROID: the cut's area centroid (cut_centroid).  SH_SEAT_SPHERE_AXIS: the fitted sphere's centre
 *                   projected onto the plane; a cut whose sphere_status != 0 gets that status in its seats (a ring over an empty
 *                   head piece, which has no sphere: SH_ERR_GEOMETRY).  seat_center = o + s_u u + s_w w with (s_u, s_w) the
 *                   in-plane coordinates of that point about o.
 *   covered_area    area(polygon n disk), exact, edge by edge by Green's theorem about s: for the directed edge p -> q with a = p - s,
 *                   d = q - p solve |a + t d|^2 = rho^2; with a positive discriminant and roots t_lo < t_hi the part of [0, 1] inside
 *                   [t_lo, t_hi] is the chord piece and contributes cross(x, y) / 2 (x, y the piece's ends about s); every other
 *                   piece contributes the sector rho^2 atan2(cross(x, y), dot(x, y)) / 2, and so does the whole edge when the
 *                   discriminant is <= 0 (a tangent edge counts as outside).  Pieces are classified by the roots, never by testing
 *                   a midpoint.  |sum over the ring|.  (sh_scalar.h seat_edge_term.)
 *   coverage = covered_area / cut_area (0 for a loop without area), overhang_area = pi rho^2 - covered_area (disk beyond the bone),
 *   uncovered_area = cut_area - covered_area (bone beyond the disk).
 *   rim_min         the smallest point-to-segment distance from s to the ring, the first segment in ring order winning a tie;
 *   rim_max         the largest vertex distance from s (the distance is convex along a segment), the first vertex winning a tie;
 *                   max_overhang = max(0, rho - rim_min), max_uncovered = max(0, rim_max - rho); overhang_dir / uncovered_dir: unit
 *                   CT vectors from s to that nearest point / farthest vertex (zero when s lies on it).  These are RADIAL measures
 *                   about s -- how far the disk's rim lies from the ring along rays from s -- NOT Hausdorff distances between
 *                   the two outlines.
 *   center_inside   1 when the winding number of s in the ring is non-zero, else 0.
 *   implant_center = s + (h - R) n^ (CT): the centre of the implant's sphere when its base lies in the plane, the dome on the
 *                   normal's side.  cor_shift = implant_center - sphere_center (CT; zero when the cut has no sphere);
 *                   cor_shift_articular = that vector rotated by csys_articular (rotation part), NaN exactly where
 *                   sh_head_fit.center_articular is.
 *   surface_rms     sqrt(sum w (|p - c|^2 - R^2)^2 / S0) / (2 R) over the head piece's samples (see sh_head_fit) against the implant
 *                   sphere (c = implant_center, R): the first-order radial rms, sphere_rms' formula, evaluated from the sixteen
 *                   moments only and about their weighted centroid (sh_scalar.h seat_surface_rms); 0 for an empty piece.
 *   status          the cut's ring status (sh_resection.status), the humerus' failed record, or in SH_SEAT_SPHERE_AXIS mode the
 *                   sphere's status.  ALL other fields are zero when it is non-zero, and also for a cut without a loop (status 0).
 *                   A bad seat never fails the batch.
 * A seat record depends on its cut and its head alone: not on B, P, K, the humerus' position in the batch or the head's in the
 * catalogue (sums are taken lane-strided in ring order and reduced by one fixed tree; no floating-point atomics). */
#define SH_SEAT_CUT_CENTROID 0
#define SH_SEAT_SPHERE_AXIS 1
#define SH_SEAT_MAX_HEADS 64
typedef struct sh_implant_head { double radius, thickness; } sh_implant_head;
typedef struct sh_seat {
  double base_radius, seat_center[3];
  double covered_area, coverage, overhang_area, uncovered_area;
  double rim_min, rim_max, max_overhang, max_uncovered;
  double overhang_dir[3], uncovered_dir[3];
  double implant_center[3], cor_shift[3], cor_shift_articular[3];
  double surface_rms;
  int32_t center_inside, status;
} sh_seat;
/* sh_resect_planes_fit / sh_resect_offsets_fit with K heads seated on every cut: same preconditions, argument checks and state
 * errors; `out` and `fit_out` are byte-equal to what the _fit calls write.  seat_out: B x P x K, host.  SH_ERR_ARG for K outside
 * 1..SH_SEAT_MAX_HEADS, a head that is not valid (non-finite, or thickness outside (0, 2 radius)) or a center_mode other than
 * the two above.  The passes of a sweep are the fitted calls' (4 096 / B planes, at least one; the ring coordinates of a pass take
 * 16 KB per cut: 64 MB for B <= 4 096, 16 KB per humerus beyond); the pass a cut falls into does not change its records.  The
 * B x P x K records (232 B each) are held on the device as well and are not limited: SH_ERR_NOMEM when they do not fit. */
int sh_resect_planes_seat (sh_ctx*, const double* planes, int P, const sh_implant_head* heads, int K, int center_mode,
                           sh_resection* out, sh_head_fit* fit_out, sh_seat* seat_out /* B x P x K */);
int sh_resect_offsets_seat(sh_ctx*, const sh_cut_offset* offs, int P, const sh_implant_head* heads, int K, int center_mode,
                           sh_resection* out, sh_head_fit* fit_out, sh_seat* seat_out /* B x P x K */);

/* ---- canal profiles and the fit of a catalogue of stems below every cut ----------------------------------------------------
 * The other half of the step the reference leaves open (arthroplasty.py:178-182, the commented-out `HumeralImplantation` that
 * "continues from the humeral head osteotomy and places the implant"): how wide the bone is around the canal axis below a cut,
 * and which stems of a catalogue go down there.  Both on the device from the resident float32 mesh (k_stem.h); no section of the
 * mesh goes to the host.
 *
 * Canal frame of humerus b: a rigid 4 x 4 matrix T (row-major, CT -> frame), the caller's or the record's csys_articular (origin
 * at the canal-axis midpoint, z the canal pointing proximally, x / y posterior-anterior / lateral-medial).  A vertex is widened
 * to float64 and mapped as ((T[4i] x + T[4i+1] y) + T[4i+2] z) + T[4i+3] (sh_scalar.h canal_map_point).
 *   grid      level l is the plane z = z_l = z0 - l dz of the frame (dz > 0: levels run distally), l < L; ray (l, a) starts at
 *             (0, 0, z_l) and goes along (cos t_a, sin t_a, 0), t_a = (2 pi a) / A, a < A.  The A directions are computed once
 *             on the host and every kernel reads that table ("canal.dirs").
 *   hit rule  Moller-Trumbore as SH_STAGE_ANP's rays state it (k_anp.h k_rays_hit; sh_scalar.h canal_ray_hit): |det| > 1e-12,
 *             u >= 0, w >= 0, u + w <= 1 (closed), t > 1e-9.  near[b][l][a] is the smallest t over ALL faces of humerus b, far the
 *             largest; no hit: near = +inf, far = 0.  Minimum and maximum do not depend on an order: a humerus' rows are the same
 *             bits whatever the batch, its position in it, L or the tiling.  Named buffers "canal.near" / "canal.far"
 *             (B x L x A doubles, sh_fetch), valid until the next upload / commit.
 *   level     r_a = near[l][a], p_a = r_a (cos t_a, sin t_a).  r_min / r_max with their angle indices (the smaller index wins a
 *             tie), r_mean = sum r_a / A, area = (0.5 sin(2 pi / A)) sum r_a r_(a+1), centroid = sum (p_a + p_(a+1)) c_a /
 *             (3 sum c_a) with c_a = cross(p_a, p_(a+1)) (zero when sum c_a is), extent_x / extent_y = [min, max] of the p_a's
 *             coordinates, wall_min = min (far - near), n_hit = rays with a hit.  Sums are taken lane-strided in angle order by
 *             one wave and added by one fixed shuffle tree.  A level with n_hit < A has status SH_ERR_GEOMETRY, n_hit valid and
 *             every other field zero; a humerus whose record failed (frames == NULL) has that status in all of its levels,
 *             near = +inf and far = 0.  A bad level never fails the batch. */
typedef struct sh_canal_grid { double z0, dz; int32_t L, A; } sh_canal_grid;
typedef struct sh_canal_level {
  double r_min, r_max, r_mean, area, centroid[2], extent_x[2], extent_y[2], wall_min;
  int32_t a_min, a_max, n_hit, status;
} sh_canal_level;
/* L in 1..1024, A in 3..256; a non-finite value, dz <= 0 or a frame that is not rigid (non-finite, rotation rows not orthonormal
 * to 1e-9, determinant not positive, last row not 0 0 0 1): SH_ERR_ARG.  frames == NULL needs a collected run of the resident
 * batch with SH_STAGE_ANP | SH_STAGE_CSYS (SH_ERR_STATE otherwise, as sh_resect_offsets); explicit frames need a resident batch
 * only.  Not while runs are in flight (SH_ERR_STATE).  Every output pointer may be NULL. */
int sh_canal_profile(sh_ctx*, const sh_canal_grid* grid, const double* frames /* B x 16, or NULL: each record's csys_articular */,
                     double* near_out /* B x L x A, host */, double* far_out /* B x L x A, host */, sh_canal_level* levels_out /* B x L, host */);

/* A stem is a frustum about the canal axis: r(d) = r_prox + ((r_tip - r_prox) d) / length at depth 0 <= d <= length below its
 * entry point (sh_scalar.h stem_radius_at).  sh_resect_stems fits K stems below each of the B x P planes of the LAST
 * sh_resect_* call against the LAST sh_canal_profile of the same resident batch (SH_ERR_STATE when either is missing or a new
 * batch was uploaded since); K in 1..SH_STEM_MAX, every number of a stem finite and > 0 (SH_ERR_ARG).  Per (b, p, k), with the
 * plane (o, n) mapped into the frame and n^ = n / |n| there:
 *   entry     where the frame's z axis pierces the plane: z_entry = o_z + (o_x n^_x + o_y n^_y) / n^_z, `entry` the point in CT.
 *             |n^_z| < 1e-12: status SH_ERR_GEOMETRY.
 *   levels    the levels with 0 <= d_l <= length, d_l = z_entry - z_l.  A grid that does not reach from z_entry down to
 *             z_entry - length (z0 < z_entry or z_(L-1) > z_entry - length): status SH_ERR_ARG, nothing is extrapolated.
 *   samples   (l, a) of a used level counts when the stem's surface point q = (r(d_l) cos t_a, r(d_l) sin t_a, z_l) lies on the
 *             retained side, dot(q - o, n^) <= 0 (the head piece is on the normal's side, as everywhere in sh_resection).
 *   min_clearance = min (near - r(d_l)) over the counted samples that have a hit, with its `depth` d_l, `angle_index` a and
 *             `direction` (the ray's unit direction in CT); the smaller (l, a) wins a tie.  scale_max = min near / r(d_l): the
 *             largest uniform radial scale of the stem that still clears.  Without such a sample: 0, 0, -1, zeros, 0.
 *   n_samples counted samples, n_breach those with near - r < 0, n_open those without a hit.
 *   fill      pi r(d_l)^2 / area_l over the used levels whose sh_canal_level.status is 0 and whose area is > 0: fill_mean (added
 *             in level order by one lane), fill_max with fill_max_depth (the first level wins a tie); zeros without such a level.
 *   fits      1 when n_breach = 0, n_open = 0 and n_samples > 0.
 *   status    the humerus' failed record or profile frame, the cut's status (sh_resection.status) or one of the two above; every
 *             other field is zero then.  A bad record never fails the batch.
 * A record depends on its cut, its stem and the profile alone: not on B, P, K or the stem's place in the catalogue (lanes stride
 * the samples in (l, a) order, minima carry their sample index through one fixed shuffle tree; no floating-point atomics). */
#define SH_STEM_MAX 64
typedef struct sh_stem { double length, r_prox, r_tip; } sh_stem;
typedef struct sh_stem_fit {
  double entry[3], z_entry;
  double min_clearance, depth, direction[3], scale_max;
  double fill_mean, fill_max, fill_max_depth;
  int32_t angle_index, n_samples, n_breach, n_open, fits, status;
} sh_stem_fit;
int sh_resect_stems(sh_ctx*, const sh_stem* stems, int K, sh_stem_fit* out /* B x P x K, host */);

/* ---- implant plans: cuts, heads and stems joined and ranked -------------------------------------------------------------------
 * The step the four calls above were built for (arthroplasty.py:178-182, the commented-out `HumeralImplantation` that "continues from
 * the humeral head osteotomy and places the implant"): the N best (cut, head, stem) triples of every humerus under one rule, ranked
 * on the device from the records of the LAST seated call (sh_resect_*_seat, K_h heads) and the LAST sh_resect_stems (K_s stems) of
 * the resident batch (k_plan.h).  No record goes to the host for it, and the ranking is the same bytes wherever it is run.
 *
 * Frame of humerus b: "canal.frames"[b] of the last sh_canal_profile, the frame the stems were fitted in; a point maps as
 * sh_canal_profile maps a vertex (sh_scalar.h canal_map_point), "the frame's z" is the third coordinate of that.
 *
 * sh_plan_ref, the reference of a humerus.  The reference plane (o_a, n_a) is row b of ref_planes or, with ref_planes == NULL, the
 * anp_plane_point / anp_plane_normal of the humerus' record.  For each vertex v of the humerus, widened to float64:
 * s_v = ((v_x - o_x) n_x + (v_y - o_y) n_y) + (v_z - o_z) n_z with the normal as given, z_v the frame's z of v.
 *   head_apex        the vertex with s_v > 0 and the largest z_v; head_apex_z its z_v, head_apex_vid its index in the humerus
 *   tuberosity_top   the vertex with s_v <= -(margin |n_a|) and the largest z_v (margin: sh_plan_rule, mm); tuberosity_z, tuberosity_vid
 *                    Of equal z_v the smaller vertex index wins, on both sides.
 *   head_height      head_apex_z - tuberosity_z
 *   n_feasible       the number of ALL feasible candidates of the humerus (see below), not of the returned ones
 *   status           SH_ERR_GEOMETRY when a side has no vertex; the status of a failed record (ref_planes == NULL; SH_ERR_GEOMETRY for a
 *                    record whose plane is not finite) or of a failed "canal.status"[b].  With a non-zero status every other field is
 *                    zero, the vids are -1, n_feasible is 0 and all N plans of the humerus carry the status.
 * On an intact humerus with a true anatomic-neck plane, tuberosity_top is the top of the greater tuberosity: the highest point of
 * the bone along the canal that is not head.  This is a GEOMETRIC definition.  Nobody has checked it against annotated anatomy, and
 * the anatomic-neck network that ships with this library is a seeded stand-in, not a trained one.
 *
 * A candidate of humerus b is (p, k_h, k_s) with index i = (p K_h + k_h) K_s + k_s.  Its cost is the sum of three parts, every sum
 * added left to right as written:
 *   cut part (b, p)       entry: where the frame's z axis pierces the cut's plane, sh_resect_stems' `entry` (sh_scalar.h stem_entry).
 *                         eccentricity = |seat_center - entry| (sh_seat.seat_center of the cut: how far the head's taper would sit
 *                         from the stem's axis, in the plane); cut_cost = w_eccentricity eccentricity.  Feasible when
 *                         sh_resection.status == 0, n_loops >= 1, the seat record k_h = 0 of the cut has status 0 (a seat's status and
 *                         seat_center depend on the cut alone), the entry exists, sphere_status == 0 when w_cor > 0, and
 *                         eccentricity <= max_eccentricity.
 *   head part (b, p, k_h) uncovered = 1 - coverage, overhang = max_overhang, cor = |cor_shift| (all of sh_seat), apex = seat_center +
 *                         (h n) / |n| with h the head's thickness and n the cut's normal, apex_z the frame's z of apex, height =
 *                         |apex_z - head_apex_z|; head_cost = ((w_uncovered uncovered + w_overhang overhang) + w_cor cor) + w_height
 *                         height.  Feasible when max_overhang <= rule.max_overhang and coverage >= min_coverage.
 *   stem part (b, p, k_s) fill = |fill_mean - fill_target|, stem_cost = w_fill fill.  Feasible when status == 0, fits == 1 and
 *                         min_clearance >= rule.min_clearance (all of sh_stem_fit).
 *   cost = (head_cost + stem_cost) + cut_cost.  The candidate is feasible when its three parts are, its cost is not NaN and compat ==
 *   NULL or bit k_s of compat[k_h] is set (which stems of a system a head goes with).
 * Candidates sort ascending by (cost, i); plan r of a humerus is its r-th feasible candidate in that order.  A slot beyond
 * n_feasible has cut = head = stem = -1, status SH_ERR_GEOMETRY and every other field zero.
 *
 * sh_plan: cost and its six UNWEIGHTED terms, the apex of the implant head (CT), its frame height, head_height = apex_z -
 * tuberosity_z (the restored head height above the tuberosity, to be read against sh_plan_ref.head_height), the three indices.
 *
 * SH_ERR_ARG: N outside 1..SH_PLAN_MAX, a NULL rule or out, a NaN anywhere in the rule, a weight that is negative or infinite,
 * margin < 0, a ref_planes row that is not finite or has a zero normal.  A limit of +-inf switches that limit off.
 * SH_ERR_STATE (sh_last_error names what is missing): no seated resection of the resident batch; stems that were not fitted
 * against exactly that resection and the current profile (a resection or a profile made after sh_resect_stems voids the stems FOR
 * THIS CALL only: sh_resect_stems itself keeps its preconditions); ref_planes == NULL without a collected run with SH_STAGE_ANP |
 * SH_STAGE_CSYS; runs in flight.  SH_ERR_NOMEM when the buffers do not fit.  A bad plan never fails the batch.
 *
 * Named buffers (sh_fetch), valid until the next upload / commit / sh_store("verts") as the profile is: "plan.ref" (B sh_plan_ref),
 * "plan.out" (B x N sh_plan), and the compact parts of 16 bytes {double cost; int32 feasible; int32 pad}: "plan.cut_terms" (B x P),
 * "plan.head_terms" (B x P x K_h), "plan.stem_terms" (B x P x K_s).
 * Determinism: the vertex maxima are reduced per tile of 256 vertices by one fixed tree and the tiles in tile order; the ranking
 * takes N rounds of an arg-min of the key (cost, i) over the keys greater than the previous round's.  Maxima and minima under a total
 * order do not depend on the reduction order: a humerus' rows are the same bytes whatever B, its position in the batch or the launch
 * shape.  No floating-point atomics, no floating-point sums across lanes.
 * Cost: one pass over the vertices and N P K_h K_s / 256 two-load evaluations per lane of one workgroup per humerus -- nothing at
 * a planning sweep (27 x 16 x 16, N = 8), slow at the limits (4 096 x 64 x 64, N = 64: 4e6 evaluations per lane).  There is one
 * variant. */
#define SH_PLAN_MAX 64
typedef struct sh_plan_rule {            /* 12 doubles */
  double max_overhang, min_coverage, min_clearance, max_eccentricity;   /* limits; +-inf switches one off */
  double fill_target, margin;            /* margin >= 0, mm: see sh_plan_ref */
  double w_uncovered, w_overhang, w_cor, w_height, w_eccentricity, w_fill;   /* finite, >= 0 */
} sh_plan_rule;
typedef struct sh_plan_ref {             /* one per humerus, 96 B */
  double tuberosity_top[3], tuberosity_z, head_apex[3], head_apex_z, head_height;
  int64_t n_feasible;
  int32_t tuberosity_vid, head_apex_vid, status, pad;
} sh_plan_ref;
typedef struct sh_plan {                 /* one per (humerus, rank), 112 B: twelve doubles and four int32, no padding */
  double cost, uncovered, overhang, cor, height, eccentricity, fill;    /* cost and its six UNWEIGHTED terms */
  double apex[3], apex_z, head_height;
  int32_t cut, head, stem, status;
} sh_plan;
int sh_resect_plan(sh_ctx*, const sh_plan_rule* rule, const uint64_t* compat /* K_h words or NULL */,
                   const double* ref_planes /* B x (point, normal), CT, or NULL: each record's anp plane */,
                   int N, sh_plan* out /* B x N, host */, sh_plan_ref* ref_out /* B, host, nullable */);

/* ---- rays against the resident batch: every hit, ordered ----------------------------------------------------------------------
 * The reference asks `ray.intersects_location` (anatomic_neck.py:184-192, 217-224), which returns every hit; SH_STAGE_ANP keeps the
 * nearest forward hit of its four rays (canonical rule B-6) and sh_canal_profile the nearest and the farthest.  These two calls
 * return all of them: B resident humeri x R rays in one device pass (k_rays.h), brute force over the faces.
 *   ray       sh_ray: origin and direction in CT.  The direction need not be a unit vector: t counts in units of |dir|.  A
 *             non-finite number or a zero direction: SH_ERR_ARG.
 *   hit rule  sh_scalar.h canal_ray_hit operation by operation (which restates k_rays_hit), through ray_tri_hit, the statement
 *             that also returns det's sign: |det| > 1e-12, u >= 0, w >= 0, u + w <= 1 (closed), t > 1e-9, against the resident
 *             float32 vertices widened to float64.
 *   hit       sh_ray_hit (40 B): t; point[k] = origin[k] + dir[k] * t (the form of SH_STAGE_ANP's axis points); face, the
 *             humerus-local face id; side = +1 when det > 0 -- the ray runs against the face's normal, so it ENTERS a mesh whose
 *             normals point outward -- and -1 otherwise.  A ray through a shared edge or vertex hits every face the closed rule
 *             accepts, and all of those hits are kept.
 *   order     ascending by (t, face): a total order, so the result does not depend on the order the hits were found in (rule B-6
 *             extended: "ascending t, then face").
 *   counts    counts[b][r] is the exact number of hits over all faces whatever `cap` is; the first min(count, cap) hits in order
 *             are stored and the slots behind them are zero with face = -1, so a smaller cap gives a byte prefix of a larger one.
 *             cap in 1..SH_RAY_MAX_HITS, R in 1..SH_RAY_MAX (SH_ERR_ARG).
 * A (humerus, ray) result depends on that mesh and that ray alone: not on B, the humerus' position in the batch, R, the ray's
 * place in the list, cap, the tiling or the launch shape.  Integer atomics only choose slots of a pool and the sort removes their
 * order; no floating-point atomics, no floating-point sums across lanes.
 *
 * sh_ray_cast needs a resident batch only, not a run: SH_ERR_STATE without one or while runs are in flight, SH_ERR_NOMEM when the
 * hit pool (16 B per hit of the call) or the results do not fit.  rays: R rays shared by all humeri, or B x R with per_humerus != 0.
 * The results stay resident in the named buffers "ray.hits" (B x R x cap sh_ray_hit) and "ray.counts" (B x R int32) until the next
 * upload / commit / sh_store("verts"), as the canal profile does; both host pointers may be NULL.
 *
 * sh_anp_axis_hits casts the four rays of SH_STAGE_ANP (0 = +normal, 1 = -normal, 2 = +central, 3 = -central; k_anp.h ray_dir)
 * for every humerus of the last collected run, in the box frame, from "anp.plane", against the vertices as that stage read them:
 * each corner is "obb_transform" applied to the float32 vertex by the expression of the kernel that fills "verts_obb".  t is the
 * box-frame parameter and equals "anp.ray_t" for the first hit; points are mapped to CT exactly as the record's anp_axis_normal /
 * anp_axis_central rows are, so hits[b][ray][0].point equals the record's row bit for bit.  A humerus whose record failed gets its
 * status and zero counts; it never fails the batch.  Without a collected run of the resident batch that had SH_STAGE_ANP:
 * SH_ERR_STATE.  status must not be NULL; hits and counts may be.
 *
 * sh_ray_nearest returns the nearest hit only (`ray.intersects_first`, `intersects_location(multiple_hits=False)`): per (humerus,
 * ray) the minimum of all hits under (t, face) -- the bytes of hits[b][r][0] of sh_ray_cast; a ray that hits nothing gets zero with
 * face = -1.  Arguments, limits, refusals and their order are sh_ray_cast's (cap = 1).  The result stays resident as "ray.near"
 * (B x R sh_ray_hit) until the next upload / commit / sh_store("verts").  With SH_ACCEL_OFF it is the chain of sh_ray_cast with cap = 1
 * (and rewrites "ray.hits" / "ray.counts" at that cap); with SH_ACCEL_BVH it is one launch through the face hierarchy (k_raytree.h).
 *
 * With sh_set_query_accel(SH_ACCEL_BVH) sh_ray_cast and sh_ray_nearest descend the face hierarchy ("bvh.*", built first when it is not
 * resident) instead of testing every face: one ray per lane, a node skipped only when the hit rule AS COMPUTED rejects every face in it
 * (k_raytree.h states the argument).  THE RESULTS ARE THE SAME BYTES in either mode.  The rule must grow every box by what the hit
 * rule's division admits, and as measured the descent is SLOWER than the walk over all faces for rays: the switch buys
 * rays no time, only sh_ray_nearest without a host round trip.  sh_anp_axis_hits stays on the walk over all faces: its corners are the
 * vertices under "obb_transform", which the index does not hold. */
#define SH_RAY_MAX 65536
#define SH_RAY_MAX_HITS 1024
typedef struct sh_ray { double origin[3], dir[3]; } sh_ray;
typedef struct sh_ray_hit { double t; double point[3]; int32_t face; int32_t side; } sh_ray_hit;
int sh_ray_cast(sh_ctx*, const sh_ray* rays /* R, or B x R when per_humerus */, int R, int per_humerus, int cap,
                sh_ray_hit* hits /* B x R x cap, host, nullable */, int32_t* counts /* B x R, host, nullable */);
int sh_anp_axis_hits(sh_ctx*, int cap, sh_ray_hit* hits /* B x 4 x cap, host, nullable */, int32_t* counts /* B x 4, host, nullable */,
                     int32_t* status /* B, host */);
int sh_ray_nearest(sh_ctx*, const sh_ray* rays /* R, or B x R when per_humerus */, int R, int per_humerus,
                   sh_ray_hit* hit /* B x R, host, nullable */);

/* ---- closest surface points of the resident batch ------------------------------------------------------------------------------
 * The counterpart of `trimesh.proximity.closest_point(mesh, points)`: for Q query points, shared by all humeri or Q per humerus, the
 * nearest point of each of the B resident meshes, in one device pass (k_closest.h), brute force over the faces with a conservative cull.
 *   rule      sh_scalar.h closest_pt_tri: the Voronoi-region walk of Ericson, Real-Time Collision Detection 5.1.5, on the resident
 *             float32 vertices widened to float64, the triangle kept as (A, ab, ac); the regions are tested in the fixed order vertex A,
 *             vertex B, edge AB, vertex C, edge CA, edge BC, interior.
 *   winner    the smallest (d2, face) over the faces of the humerus (closest_key_less): a total order, so the result does not depend on
 *             the order the faces were walked in.  A point whose nearest feature is an edge or a vertex sees the same d2 from every
 *             incident face: the smallest face id wins.  A d2 that is not finite never wins.
 *   sh_closest (48 B)  dist = sqrt(d2) of the winner; point = A + ab u + ac w, recomputed from the winning face alone, in CT; face, the
 *             humerus-local face id; region: 0 interior, 1 / 2 / 3 edge AB / BC / CA, 4 / 5 / 6 vertex A / B / C of that face;
 *             side = +1 when (p - point) . (ab x ac) >= 0 and -1 otherwise.  With region == 0 side says outside (+1) or inside (-1) a
 *             mesh whose normals point outward.  For an edge or a vertex winner it is the WINNING FACE's verdict, which can be wrong at
 *             sharp or saddle features (Baerentzen & Aanaes, Signed distance computation using the angle weighted pseudonormal, 2005);
 *             a robust inside test (parity, winding number) is sh_winding_numbers, below.
 *             status 0; SH_ERR_GEOMETRY (the kernels' SH_ERR_GEOMETRY_DEV) with face = -1 and every other field zero when no face of the humerus gave a finite d2.
 * A (humerus, point) result depends on that mesh and that point alone: not on B, the humerus' position in the batch, Q, the point's
 * place in the list, or how the faces were split or tiled.  No floating-point atomics, no floating-point sums across lanes.
 *
 * Arguments in this order: the context, points != NULL and Q in 1..SH_CLOSEST_MAX (SH_ERR_ARG); a resident batch and no runs in flight
 * (SH_ERR_STATE; a run is not needed); every coordinate finite (SH_ERR_ARG).  SH_ERR_NOMEM when the results or the partials do not fit.
 * The results stay resident in the named buffer "cp.out" (B x Q sh_closest) until the next upload / commit / sh_store("verts"), which
 * removes it.  The call changes nothing else: the records of a run and the buffers of the arthroplasty chain keep their bytes. */
#define SH_CLOSEST_MAX 1048576
typedef struct sh_closest { double dist; double point[3]; int32_t face, region, side, status; } sh_closest;   /* 48 B */
int sh_closest_points(sh_ctx*, const double* points /* Q x 3, or B x Q x 3 when per_humerus; CT */, int Q, int per_humerus,
                      sh_closest* out /* B x Q, host, nullable */);

/* ---- generalized winding numbers of the resident batch: inside tests --------------------------------------------------------------
 * The counterpart of `mesh.contains(points)`, and with sh_closest_points of `trimesh.proximity.signed_distance`: for Q query points,
 * shared by all humeri or Q per humerus, the generalized winding number (Jacobson, Kavan, Sorkine-Hornung, Robust inside-outside
 * segmentation using generalized winding numbers, 2013) of each of the B resident meshes, in one device pass (k_winding.h).  Every face
 * contributes: no cull, no far-field approximation.
 *   rule      sh_scalar.h solid_angle_tri (Van Oosterom & Strackee 1983) on the resident float32 corners widened to float64: with
 *             a = A - p, b = B - p, c = C - p and la, lb, lc their lengths (sqrt of dot3),
 *               num = a . (b x c)      den = ((la lb) lc + (a . b) lc) + ((a . c) lb + (b . c) la)      omega = 2.0 atan2(num, den),
 *             and omega = 0 when num == 0.0 (either zero): a point in the plane of a face gets nothing from that face.
 *   sum       w = (sum over blocks (sum over the faces of the block omega_f)) / (4 pi).  A block is SH_WIND_BLOCK = 2048 consecutive
 *             faces; a block sum starts at 0 and adds its faces in face order; the block sums are added in block order, starting at
 *             0; 4 pi is 4.0 * M_PI.  This one summation tree is part of the definition: it does not depend on B, Q, the launch shape
 *             or the face split.  No floating-point atomics, no floating-point sums across lanes.
 *   sh_winding (16 B)  winding = w.  On a closed, consistently oriented mesh w is an integer up to rounding (1 inside a mesh whose
 *             normals point outward, -1 inside one stored inside-out, 0 outside, 0 in a cavity whose wall faces inward, 2 inside a mesh
 *             stored twice); on an open mesh it is a fraction.  inside = 1 when |w| >= 0.5, else 0: the non-zero rule of
 *             sh_seat.center_inside, so a mesh stored inside-out still answers "inside".  ON THE SURFACE ITSELF w is about 0.5 and
 *             inside is undefined.  status 0; SH_ERR_GEOMETRY (the kernels' SH_ERR_GEOMETRY_DEV) with winding = 0 and inside = 0 when
 *             the sum is not finite (a point 1e200 mm away along a diagonal: the products of b x c overflow to inf - inf.  Along one
 *             axis only the lengths overflow: den is +inf, every term is 0 and w = 0 with status 0, the right answer out there).
 * A (humerus, point) result depends on that mesh and that point alone, byte for byte.  The device's atan2 is its math library's: against
 * another library's the sum differs within (2 F + 16) 2^-53 max(1, sum |omega_f| / 4 pi), F the faces.
 *
 * Arguments in this order: the context, points != NULL and Q in 1..SH_WINDING_MAX (SH_ERR_ARG); a resident batch and no runs in flight
 * (SH_ERR_STATE; a run is not needed); every coordinate finite (SH_ERR_ARG).  SH_ERR_NOMEM when the results or the partials do not fit.
 * The results stay resident in the named buffer "wn.out" (B x Q sh_winding) until the next upload / commit / sh_store("verts"), which
 * removes it.  The call changes nothing else: the records of a run and the buffers of the arthroplasty chain keep their bytes. */
#define SH_WINDING_MAX 1048576
#define SH_WIND_BLOCK 2048
typedef struct sh_winding { double winding; int32_t inside, status; } sh_winding;   /* 16 B */
int sh_winding_numbers(sh_ctx*, const double* points /* Q x 3, or B x Q x 3 when per_humerus; CT */, int Q, int per_humerus,
                       sh_winding* out /* B x Q, host, nullable */);

/* ---- rigid registration of point sets onto the resident batch (ICP) ----------------------------------------------------------------
 * The counterpart of `trimesh.registration.icp(points, mesh)` / `mesh.register`: for B humeri x Q points, up to max_iter rigid ICP
 * iterations per humerus, the whole loop on the device (k_icp.h, with the unchanged k_cp_walk / k_cp_join), one transform per humerus
 * with its evidence.  ICP is LOCAL: it needs an initial pose inside its basin of convergence; no global search is made here
 * (sh_register_multistart, below, makes one on top of this call).
 *   options   metric SH_ICP_POINT (Horn's closed form per iteration, linear convergence) or SH_ICP_PLANE (linearised point-to-plane,
 *             quadratic near the solution); max_iter in 1..64; reject in mm, > 0, +inf accepts every pair; tol >= 0, 0 runs every
 *             iteration.
 *   T0        B x 16 row-major CT -> CT, NULL for the identity.  Must be rigid: last row exactly (0, 0, 0, 1), |R^T R - I|_inf <= 1e-9
 *             (the 1e-9 is part of the definition), det > 0.
 * ONE EVALUATION k = 0 .. max_iter of humerus b at its current T (everything float64, -ffp-contract=off; sh_scalar.h):
 *   move      p'_i = T p_i, row r: ((T[4r] x + T[4r+1] y) + T[4r+2] z) + T[4r+3] (canal_map_point).
 *   pair      the sh_closest of p'_i on mesh b, the rule of sh_closest_points unchanged (ties to the smallest face id).
 *             e_i = q_i - p'_i, e2_i = dot3(e_i, e_i).  ACCEPTED when its status is 0 and sqrt(e2_i) <= reject.  Plane metric:
 *             n_i = (ab x ac) / sqrt(dot3(ab x ac, ab x ac)) of the winning face whatever the region; a face of zero area is not accepted.
 *   sum       a pair that is not accepted contributes +0.0 to every term.  THE TREE IS PART OF THE DEFINITION: points in blocks of
 *             SH_ICP_BLOCK = 256 consecutive indices; in a block slot[i] += slot[i + h] for h = 128, 64, .., 1 (missing points of the
 *             last block are +0.0); the block sums added in block order starting at 0.0.  No floating-point atomics, nothing that
 *             depends on B, the launch shape or the split of the walk.  Terms: n, sum e2; point metric sum p', sum q, sum p'_i q_j
 *             (9); plane metric, with d_i = p'_i - c, J_i = (d_i x n_i, n_i), r_i = dot3(e_i, n_i): the 21 upper terms of sum J J^T
 *             and the 6 of sum J r.  The pivot c = T cbar, cbar = (sum p_i) / Q over ALL Q input points of the humerus by the same
 *             tree, once, before the first evaluation.
 *   report    rms_k = sqrt(sum e2 / n) (0 when n = 0), pairs_k = n.
 *   stop/step in this order: k > 0 and |rms_{k-1} - rms_k| <= tol: converged = 1, stop; k == max_iter: stop; n < 6 or the solve fails:
 *             SH_ERR_GEOMETRY, stop; else T <- (dR, dt) T (icp_compose).  The reported rms and pairs always belong to the returned T:
 *             no update is applied after the last evaluation, and after a failure T is the transform that evaluation was made at
 *             (T0 when the first one failed).
 *   solve, point   icp_horn_solve: pbar = sum p' / n, qbar = sum q / n, S_ij = sum p'_i q_j - (sum p'_i) qbar_j, Horn's symmetric 4 x 4,
 *             its largest eigenvector by sym4_jacobi (12 cyclic sweeps, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
 *             t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)); among equal eigenvalues the first), the quaternion normalised with
 *             w >= 0, dt = qbar - R pbar.  A matrix that is not finite is a failure.
 *   solve, plane   chol6_solve: Cholesky of the 6 x 6 in index order; a pivot <= 0 or not finite is a failure.  x = (w, t); dR is the
 *             rotation of the quaternion (1, w / 2) normalised (no sin, no cos: the chain is + - x / sqrt), dt = (c - dR c) + t.
 *             min_pivot = min_j (L_jj^2 / A_jj) of the LAST solve made, in (0, 1]: small where the target lets the points slide (a
 *             plane, a sphere, a cylinder).  ONLY EXACT SINGULARITY IS A STATUS; a nearly singular system is solved and shows in
 *             min_pivot alone.  1.0 under the point metric and before any solve.
 *   sh_registration (168 B)  T; rms, pairs of the last evaluation; rms_first of evaluation 0; min_pivot; iterations, the number of
 *             updates applied; converged; status 0 or SH_ERR_GEOMETRY.  history (optional): B x (max_iter + 1) x (rms, pairs), row k
 *             of every evaluation made, zeros behind.
 * A result for (humerus, point set, T0, options) depends on those alone, byte for byte: not on B, the humerus' place, shared or
 * per-humerus points, or the walk's split.
 *
 * Arguments in this order: the context and the pointers points and options (SH_ERR_ARG); Q in 1..SH_CLOSEST_MAX; the options;
 * a resident batch and no runs in flight (SH_ERR_STATE; a run is not needed); every coordinate finite, naming the first bad point; T0,
 * naming the humerus (all SH_ERR_ARG).  SH_ERR_NOMEM when the buffers do not fit.  Resident afterwards: "icp.out" (B sh_registration),
 * "icp.near" (B x Q sh_closest, the pairs of the last evaluation: per-point residuals), "icp.moved", "icp.part", "icp.T", "icp.hist",
 * "icp.flags"; upload / commit / sh_store("verts") remove "icp.out" and "icp.near".  The call changes nothing else: "cp.out", "wn.out",
 * the records of a run and the buffers of the arthroplasty chain keep their bytes. */
#define SH_ICP_POINT 0
#define SH_ICP_PLANE 1
#define SH_ICP_BLOCK 256
#define SH_ICP_MAX_ITER 64
typedef struct sh_icp_options { int32_t metric; int32_t max_iter; double reject; double tol; } sh_icp_options;   /* 24 B */
typedef struct sh_registration { double T[16]; double rms; double rms_first; double min_pivot; int32_t pairs, iterations, converged, status; } sh_registration;   /* 168 B */
int sh_register_points(sh_ctx*, const double* points /* Q x 3, or B x Q x 3 when per_humerus; CT */, int Q, int per_humerus,
                       const double* T0 /* B x 16, nullable */, const sh_icp_options* options, sh_registration* out /* B, host, nullable */,
                       double* history /* B x (max_iter + 1) x 2, host, nullable */);

/* ---- mass properties of the resident batch: surface and volume integrals ----------------------------------------------------------
 * The counterpart of `mesh.area`, `volume`, `center_mass`, `moment_inertia`, `principal_inertia_components` and
 * `principal_inertia_vectors`, and the frame of the surface itself: for each of the B resident meshes the exact integrals over its
 * triangles, in one device pass (k_mass.h).  Everything float64, -ffp-contract=off, + - x / sqrt only (sh_scalar.h).
 *   corners   the float32 vertices widened to float64.  The pivot o is vertex 0 of the humerus' vertex array, widened: it keeps the
 *             sums from cancelling at CT coordinates.  a = A - o, b = B - o, c = C - o; ab = B - A, ac = C - A; n = cross3(ab, ac);
 *             A2 = sqrt(dot3(n, n)); s = (a + b) + c; d = dot3(a, cross3(b, c));
 *             m_ij = ((s_i s_j + a_i a_j) + b_i b_j) + c_i c_j for ij = 00, 01, 02, 11, 12, 22.
 *   terms     24 per face: [0] A2, [1..3] A2 s_k, [4..9] A2 m_ij, [10..12] n_k, [13] d, [14..16] d s_k, [17..22] d m_ij,
 *             [23] 1.0 when A2 == 0.0, else 0.0.
 *   sum       THE TREE IS PART OF THE DEFINITION and is that of sh_register_points: faces in blocks of SH_MASS_BLOCK = 256 consecutive
 *             indices; in a block slot[i] += slot[i + h] for h = 128, 64, .., 1 (missing faces of the last block are +0.0); the block
 *             sums added in block order starting at 0.0.  No floating-point atomics, nothing that depends on B, the launch shape or
 *             the humerus' place in the batch.
 *   finish    (mass_finish) with T the totals and a primed quantity relative to o.  Shell: area = T0 / 2, cs'_k = T[1 + k] / (3 T0),
 *             shell_cov C_ij = T[4 + ij] / (12 T0) - cs'_i cs'_j, closure = sqrt(dot3(N, N)) / T0 with N = T[10..12] -- 0 on a closed
 *             mesh and about cap area / area on an open one: a NECESSARY sign of closedness, not a sufficient one.  Volume:
 *             volume = T13 / 6, SIGNED (a mesh stored inside-out gives a negative one), cm'_k = T[14 + k] / (4 T13),
 *             P_ij = T[17 + ij] / 120, S_ij = P_ij - (volume cm'_i) cm'_j, the inertia tensor at density 1 about the centre of mass
 *             I_00 = S_11 + S_22, I_11 = S_00 + S_22, I_22 = S_00 + S_11, I_ij = -S_ij.  Centroids are reported in CT (+ o).
 *   frames    sym3_jacobi, the conventions of sym4_jacobi: 12 cyclic sweeps, pairs (0,1) (0,2) (1,2), the same t, among equal
 *             eigenvalues the first.  principal: the moments of I ascending with their axes; shell_eig / shell_axes: the eigenvalues
 *             of C DESCENDING with their axes, the long axis first.  Axes are rows.  Each of the first two is signed so that its
 *             component of largest magnitude is positive (the first among equals); the third is cross3(first, second).
 *   sh_mass (400 B)  faces; degenerate = T23, the faces of zero area; status SH_ERR_GEOMETRY when there are no faces, T0 == 0 or a
 *             shell quantity is not finite (the shell fields are then zero); vstatus the same for T13 == 0 or a volume quantity that is
 *             not finite (the volume fields -- volume, center_mass, inertia, principal, principal_axes -- are then zero).
 * A record depends on that mesh alone, byte for byte: not on B or the humerus' place in the batch.
 *
 * Needs the context (SH_ERR_ARG), a resident batch and no runs in flight (SH_ERR_STATE; a run is not needed).  SH_ERR_NOMEM when the
 * buffers do not fit.  The results stay resident in "mass.out" (B sh_mass) and "mass.part" (B x blocks of the largest humerus x 24
 * doubles, the block rows; zeros behind a smaller humerus' blocks) until the next upload / commit / sh_store("verts"), which removes
 * them.  The call changes nothing else. */
#define SH_MASS_BLOCK 256
typedef struct sh_mass {
  double area, volume, closure;
  double shell_centroid[3], shell_cov[6], shell_eig[3], shell_axes[9];
  double center_mass[3], inertia[9], principal[3], principal_axes[9];
  int32_t faces, degenerate, status, vstatus;
} sh_mass;   /* 400 B */
int sh_mass_properties(sh_ctx*, sh_mass* out /* B, host, nullable */);

/* ---- global registration: K starts per humerus, a short ICP on each, a final ICP from the best ---------------------------------------
 * The counterpart of `trimesh.registration.mesh_other`: where sh_register_points needs a start within its basin, this call takes K
 * starts per humerus (Engine.principal_starts makes them from the principal frames of sh_mass_properties), runs a coarse registration
 * from each and a fine one from the best.  THE RESULT IS DEFINED ENTIRELY BY CALLS OF sh_register_points, so its bytes are defined there:
 *   coarse set   Qc = min(coarse_points, Q) points (coarse_points == 0: all Q); point j of it is input point floor(j Q / Qc) in integer
 *             arithmetic (of the humerus' own Q points when per_humerus).
 *   candidate k  coarse_out[b][k] equals what sh_register_points(coarse set, T0 = T0s[b][k], coarse) returns for humerus b, byte for
 *             byte -- the pivot's mean is taken over the coarse set.
 *   winner    the smallest (rms, k) among the candidates with status 0, pairs >= min_pairs and an rms that is not NaN; min_pairs >= 6.
 *   no winner out[b] is zero but for status = SH_ERR_GEOMETRY and T = T0s[b][0]; winner[b] = -1.  The humerus takes no part in the
 *             fine stage and never fails the batch.
 *   fine      out[b] equals what sh_register_points(all Q points, T0 = coarse_out[b][winner[b]].T, fine) returns, byte for byte.
 * The K starts run one after the other on the context's stream, each the unchanged chain of sh_register_points, and the host looks
 * at nothing in between (k_ms.h: k_ms_seed puts start k in place, k_ms_pick keeps the candidate and folds it into the best).
 *
 * Arguments in this order: the context and the pointers points, T0s, coarse, fine (SH_ERR_ARG); Q in 1..SH_CLOSEST_MAX; K in
 * 1..SH_MS_MAX_STARTS, coarse_points >= 0 and min_pairs >= 6; the coarse options, then the fine ones; a resident batch and no runs in
 * flight (SH_ERR_STATE); every coordinate finite, naming the first bad point; every T0s[b][k] under the rule of T0, naming the humerus
 * and the start (all SH_ERR_ARG).  SH_ERR_NOMEM when the buffers do not fit.  Resident afterwards: "ms.coarse" (B x K
 * sh_registration), "ms.winner" (B int32), "ms.best" (B doubles: the winners' coarse rms), and the "icp.*" buffers of the FINE stage as
 * sh_register_points leaves them ("icp.near" of a humerus without a winner is not defined).  An earlier call's "icp.*" are
 * overwritten; "cp.out", "wn.out", "mass.out", the records of a run and the buffers of the arthroplasty chain keep their bytes. */
#define SH_MS_MAX_STARTS 64
int sh_register_multistart(sh_ctx*, const double* points /* Q x 3, or B x Q x 3 when per_humerus; CT */, int Q, int per_humerus,
                           const double* T0s /* B x K x 16 */, int K, const sh_icp_options* coarse, int coarse_points, int min_pairs,
                           const sh_icp_options* fine, sh_registration* out /* B, host, nullable */,
                           sh_registration* coarse_out /* B x K, host, nullable */, int32_t* winner /* B, host, nullable */);

/* ---- surface samples of the resident batch: area-weighted, thinned to a minimum spacing if asked ------------------------------------
 * The counterpart of `trimesh.sample.sample_surface` and `sample_surface_even`: N points on the surface of each of the B resident
 * meshes, every face drawn in proportion to its area, and with radius > 0 the greedy thinning of `remove_close` on top, in one device
 * pass (k_sample.h).  The producer of the points that the closest-point, winding and registration calls take.  Everything float64,
 * -ffp-contract=off, + - x sqrt only (sh_scalar.h); corners are the float32 vertices widened to float64.
 *   areas     A2_f = sqrt(dot3(n, n)), n = cross3(B - A, C - A): the expression of sh_mass_properties (face_area2).
 *   cdf       "samp.cdf", nf doubles per humerus (humerus b at its face offset).  THE ORDER IS PART OF THE DEFINITION: faces in blocks
 *             of SH_SAMPLE_BLOCK = 256 consecutive indices; in a block s[0] = A2[0], s[i] = s[i - 1] + A2[i], strictly in index order;
 *             base_0 = 0.0, base_(k+1) = base_k + s_k[255] ("samp.base", one double per block); cdf[f] = base_k + s_k[i];
 *             total = cdf[nf - 1].  Sequential on purpose: cdf is then non-decreasing in floating point, which the search needs and a
 *             tree or a Hillis-Steele scan does not give; a face of zero area has cdf[f] == cdf[f - 1] exactly.
 *   words     SplitMix64 as a counter generator: w(seed, n) = mix(seed + (n + 1) 0x9E3779B97F4A7C15) mod 2^64 with
 *             mix(z): z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31, and
 *             unit(w) = (w >> 11) 2^-53 in [0, 1).  Sample j of humerus b uses seeds[b] and the words 3j, 3j + 1, 3j + 2, nothing
 *             else: a record depends on its mesh, its seed and j alone, not on B, N, the humerus' place or the launch shape.
 *   face      target = unit(w(3j)) total; face = the smallest f with cdf[f] > target (nf - 1 when there is none, which target < total
 *             rules out: the definition's guard).  A face of zero area is never drawn.
 *   point     r1 = unit(w(3j + 1)), r2 = unit(w(3j + 2)); when r1 + r2 > 1.0: r1 = 1.0 - r1, r2 = 1.0 - r2;
 *             point_k = A_k + (r1 ab_k + r2 ac_k); u = r1, v = r2 (barycentric weights of B and C); keep = 1 without thinning.
 *   thinning  (radius > 0) the sequential greedy rule: keep_j = 1 iff no i < j has keep_i = 1 and d2(i, j) < radius radius, with
 *             d2 = (dx dx + dy dy) + dz dz on the stored points.  The set is unique, so any schedule gives these bytes; the device runs
 *             Jacobi rounds on double-buffered states: an undecided j becomes removed when a lower neighbour was kept at the start of
 *             the round, kept when all its lower neighbours were removed (or it has none).  rounds = the rounds until none is
 *             undecided (deterministic: the rounds are Jacobi).  The host enqueues max_rounds launches and looks at nothing in
 *             between; an integer count of the undecided per humerus and round lets a workgroup return at once.  A humerus with
 *             undecided samples after max_rounds: status SH_ERR_CAPACITY, rounds = max_rounds, those samples keep = -1; never the
 *             batch.  All pairs i < j are looked at (brute force, tiles of 256 through LDS): N <= SH_SAMPLE_THIN_MAX with a radius.
 *   info      area = total / 2; kept = the samples with keep == 1; status SH_ERR_GEOMETRY when there are no faces, total == 0 or total
 *             is not finite: the humerus' records are then all zero and the batch goes on.
 *
 * Arguments in this order: the context and the pointers seeds and options (SH_ERR_ARG); N in 1..SH_SAMPLE_MAX; the options (radius
 * finite and >= 0, max_rounds in 1..SH_THIN_MAX_ROUNDS, reserved == 0, N <= SH_SAMPLE_THIN_MAX when radius > 0); a resident batch and
 * no runs in flight (SH_ERR_STATE; a run is not needed).  SH_ERR_NOMEM when the buffers do not fit.  Resident afterwards: "samp.cdf",
 * "samp.base", "samp.out" (B x N sh_sample), "samp.info" (B sh_sample_info) and "samp.state" (per humerus 64 int32 -- the undecided at
 * the start of round r in word r, the seed in words 62 and 63 -- and with a radius the two state arrays of N int32), until the next upload / commit /
 * sh_store("verts"), which removes them as it removes "mass.*".  Every other buffer keeps its bytes. */
#define SH_SAMPLE_MAX        1048576   /* N, without thinning */
#define SH_SAMPLE_THIN_MAX   65536     /* N, with thinning (all pairs are looked at) */
#define SH_SAMPLE_BLOCK      256
#define SH_THIN_MAX_ROUNDS   32
typedef struct sh_sample_options { double radius; int32_t max_rounds; int32_t reserved; } sh_sample_options;   /* 16 B; radius 0: no thinning */
typedef struct sh_sample      { double point[3]; double u, v; int32_t face; int32_t keep; } sh_sample;          /* 48 B */
typedef struct sh_sample_info { double area; int32_t kept, rounds, status, reserved; } sh_sample_info;          /* 24 B */
int sh_sample_surface(sh_ctx*, int N, const uint64_t* seeds /* B, host */, const sh_sample_options* options,
                      sh_sample* out /* B x N, host, nullable */, sh_sample_info* info /* B, host, nullable */);

/* ---- mesh topology of the resident batch: incidence, face adjacency, shells, counts -------------------------------------------------
 * How the triangles of each of the B resident meshes hang together, in one device pass (k_topo.h): the vertex -> face incidence, trimesh's
 * `face_adjacency`, the connected components of `mesh.split(only_watertight=False)` ("shells") and the counts that go with them.  Indices
 * are local to the mesh; all arithmetic is integer except the box corners, which are float32 minima and maxima.
 *   degenerate  a face is degenerate when two of its three vertex INDICES are equal.  It takes no part in anything below except
 *               faces_degenerate, its three adjacency slots (SH_ADJ_DEGENERATE) and its label (-1).
 *   incidence   "topo.vrow", int32, V_b + 1 entries per mesh at voff[b] + b: the exclusive prefix sums of the number of non-degenerate
 *               faces using each vertex.  "topo.vface", int32, 3 F_b entries per mesh at 3 foff[b]: row v = vface[vrow[v] .. vrow[v + 1])
 *               lists the faces using v in ASCENDING face index; the entries behind vrow[V_b] are -1.
 *   adjacency   "topo.adj", int32, 3 per face at 3 foff[b].  Slot e of face f concerns the undirected edge {f[e], f[(e + 1) % 3]} among the
 *               non-degenerate faces: the other face's index when exactly two faces use the edge (pairs only, as face_adjacency),
 *               SH_ADJ_BORDER when f alone uses it, SH_ADJ_NONMANIFOLD when three or more do, SH_ADJ_DEGENERATE in all three slots of a
 *               degenerate face.  A manifold edge (two uses) is INCONSISTENT when both faces traverse it in the same direction.
 *   shells      the connected components of the graph with one node per non-degenerate face and one edge per slot >= 0: faces that meet
 *               only in a vertex, or only in a non-manifold edge, are in different shells.  Shell k is the one with the k-th smallest
 *               first (lowest) face.  "topo.label", int32 per face at foff[b]: the shell index, -1 for a degenerate face.
 *   rounds      the labels are unique, so any schedule gives them; the ROUNDS are part of the record, so the schedule is fixed: Jacobi
 *               rounds of FastSV on two arrays.  p[f] = f at the start.  A round reads only the old array, forms g[u] = p[p[u]], and the
 *               new p[u] is the minimum of g[u], of every g[v] with v a neighbour of u (slot >= 0), and of every g[v] with v a neighbour
 *               of some u' that has p[u'] = u.  `rounds` counts the rounds up to and including the first one that changes nothing.  The
 *               host enqueues max_rounds launches and looks at nothing in between; the workgroups of a finished mesh return at once.  A
 *               mesh not finished after max_rounds: status SH_ERR_CAPACITY, rounds = max_rounds, n_shells = shells_written = 0,
 *               largest_shell = -1, largest_faces = 0, all its labels -1, no shell records; its incidence, adjacency and the other
 *               counts stay valid.  Never the batch.
 *   sh_topology per mesh, resident in "topo.info": vertices_used = the vertices with a non-empty row; edges = the distinct undirected edges;
 *               border_edges = those with one use; nonmanifold_edges = those with three or more; inconsistent_edges; euler =
 *               vertices_used - edges + non-degenerate faces; max_valence = the longest row; n_shells, exact whatever max_shells;
 *               shells_written = min(n_shells, max_shells); largest_shell and largest_faces, ties to the smaller index (-1 and 0 without a
 *               shell); flags bit 0 (SH_TOPO_WATERTIGHT): border_edges == 0 && nonmanifold_edges == 0 && faces_degenerate == 0, bit 1
 *               (SH_TOPO_CONSISTENT): inconsistent_edges == 0.
 *   sh_shell    the first max_shells shells of each mesh, resident in "topo.shells" (B x max_shells; the records behind shells_written are
 *               zero): first_face, faces, border_slots, nonmanifold_slots, manifold_edges = (slots >= 0) / 2, inconsistent_edges, and
 *               lo / hi, the float32 box of its faces' corners (under the order in which -0 < +0: exact under any schedule).
 *
 * Arguments in this order: the context and options (SH_ERR_ARG); max_shells in 1..SH_TOPO_MAX_SHELLS, max_rounds in 1..SH_TOPO_MAX_ROUNDS,
 * reserved == 0; a resident batch and no runs in flight (SH_ERR_STATE; a run is not needed).  SH_ERR_NOMEM when the buffers do not fit.
 * Reads "verts", "faces" and the offsets.  Resident afterwards: "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info",
 * "topo.shells" and the scratch "topo.state", "topo.cursor", "topo.tmp", "topo.p", until the next upload / commit / sh_store("verts"),
 * which removes them as it removes "mass.*" and "samp.*".  Every other buffer keeps its bytes. */
#define SH_ADJ_BORDER        (-1)
#define SH_ADJ_NONMANIFOLD   (-2)
#define SH_ADJ_DEGENERATE    (-3)
#define SH_TOPO_MAX_SHELLS   65536
#define SH_TOPO_MAX_ROUNDS   32
#define SH_TOPO_WATERTIGHT   1
#define SH_TOPO_CONSISTENT   2
typedef struct sh_topology_options { int32_t max_shells, max_rounds, reserved; } sh_topology_options;          /* 12 B */
typedef struct sh_topology {
  int32_t status, rounds, faces_degenerate, vertices_used, edges, border_edges, nonmanifold_edges, inconsistent_edges;
  int32_t euler, max_valence, n_shells, shells_written, largest_shell, largest_faces, flags, reserved;
} sh_topology;                                                                                                 /* 64 B */
typedef struct sh_shell {
  int32_t first_face, faces, border_slots, nonmanifold_slots, manifold_edges, inconsistent_edges;
  float lo[3], hi[3];
} sh_shell;                                                                                                    /* 48 B */
int sh_mesh_topology(sh_ctx*, const sh_topology_options* options, sh_topology* info /* B, host, nullable */,
                     sh_shell* shells /* B x max_shells, host, nullable */);

/* ---- vertex normals and discrete curvatures of the resident batch ---------------------------------------------------------------------
 * What the incidence of sh_mesh_topology is for (k_vert.h): per face its normal, area and angles, per vertex a unit normal that is
 * continuous across faces (trimesh's `vertex_normals`), the angle defect (`vertex_defects`), the Gaussian and the mean curvature, and
 * both after Jacobi rounds of smoothing.  Everything is float64, operation by operation; corners are widened from the resident "verts"
 * as sh_mass_properties widens them; indices are local to the mesh; "degenerate" and "row" mean what they mean in sh_mesh_topology.
 *   face record  "vert.face", 10 doubles per face at 10 foff[b]: n[3], A2, angle[3], cot[3].  n = cross3(P1 - P0, P2 - P0),
 *                A2 = sqrt(dot3(n, n)) (the expression of sh_mass_properties); at corner k, e1 = P[(k + 1) % 3] - P[k],
 *                e2 = P[(k + 2) % 3] - P[k], d = dot3(e1, e2), angle[k] = atan2(A2, d), cot[k] = d / A2.  A degenerate face, or one whose
 *                A2 is 0.0 or not finite, is FLAT: ten zeros, and it contributes to no vertex.
 *   vertex sums  every accumulator starts at 0.0 and adds one term per non-flat face f of the row of v in ASCENDING face index (the
 *                order is part of the definition); k is the corner of f that is v.  s = sum A2_f, area = s / 6.0; angle_sum = sum
 *                angle_f[k]; N = sum n_f (SH_VERT_WEIGHT_AREA) or sum (n_f / A2_f) * angle_f[k] component by component
 *                (SH_VERT_WEIGHT_ANGLE: trimesh's default); L = sum (cot_f[(k + 1) % 3] * (P_k - P_(k+2)) + cot_f[(k + 2) % 3] *
 *                (P_k - P_(k+1))), in each component the two products added to each other first, then to the accumulator.
 *   results      normal = N / sqrt(dot3(N, N)), three zeros when that root is 0.0 or not finite; defect = (border ? 3.141592653589793 :
 *                6.283185307179586) - angle_sum; gauss = defect / area; mean = dot3(L, normal) / (4.0 * area); with area == 0.0 defect,
 *                gauss and mean are 0.0.  With outward normals a sphere of radius R has mean = +1/R and gauss = +1/R^2.
 *   flags        int32: SH_VERT_USED the row is not empty; SH_VERT_BORDER one of the two slots that touch v in a face of the row is
 *                SH_ADJ_BORDER; SH_VERT_NONMANIFOLD the same for SH_ADJ_NONMANIFOLD; SH_VERT_FLAT a face of the row was skipped as flat.
 *   smoothing    smooth_rounds Jacobi rounds on two arrays, for gauss and mean separately: s'[v] = (sum_f A2_f * (((s[f0] + s[f1]) +
 *                s[f2]) / 3.0)) / (sum_f A2_f), both sums over the non-flat faces of the row in ascending order, 0.0 when the denominator
 *                is 0.0.  The raw values are kept.  The host enqueues the rounds and looks at nothing in between.
 *   only atan2   differs between two math libraries: n, A2, cot, area, the flags and, with SH_VERT_WEIGHT_AREA, the normals and mean are
 *                the same bytes wherever the rule runs.
 *
 * Arguments in this order: the context (SH_ERR_ARG); weight SH_VERT_WEIGHT_AREA or SH_VERT_WEIGHT_ANGLE and smooth_rounds in
 * 0..SH_VERT_MAX_SMOOTH (SH_ERR_ARG); a resident batch and no runs in flight (SH_ERR_STATE); the incidence of THIS batch resident
 * (SH_ERR_STATE: call sh_mesh_topology first; a topology that ran out of rounds still has its incidence and adjacency and is
 * accepted).  SH_ERR_NOMEM when the buffers do not fit.  Reads "verts", "faces", the offsets, "topo.vrow", "topo.vface", "topo.adj".
 * Resident afterwards: "vert.face"; "vert.normal", 3 doubles per vertex at 3 voff[b]; "vert.fields", SH_VERT_FIELDS doubles per vertex:
 * area, angle_sum, defect, gauss, mean, gauss_smooth, mean_smooth, 0.0 (without a round the smoothed fields equal the raw ones);
 * "vert.flags"; "vert.status", B int32: SH_ERR_GEOMETRY for a mesh without a non-flat face, whose records are all zero -- never the
 * batch; and the scratch "vert.a2", "vert.plane", "vert.state".  They are removed together with "topo.*" by the next upload / commit /
 * sh_store("verts").  Every other buffer keeps its bytes. */
#define SH_VERT_WEIGHT_AREA  0
#define SH_VERT_WEIGHT_ANGLE 1
#define SH_VERT_MAX_SMOOTH   64
#define SH_VERT_FIELDS       8
#define SH_VERT_USED         1
#define SH_VERT_BORDER       2
#define SH_VERT_NONMANIFOLD  4
#define SH_VERT_FLAT         8
int sh_vertex_fields(sh_ctx*, int weight, int smooth_rounds, double* normals /* sumV x 3, host, nullable */,
                     double* fields /* sumV x SH_VERT_FIELDS, host, nullable */, int32_t* flags /* sumV, host, nullable */,
                     int32_t* status /* B, host, nullable */);

/* ---- geodesic distances and shortest paths on the resident batch -------------------------------------------------------------------------
 * What a planner asks of landmarks that lie on a surface, measured ALONG it (k_geo.h): from K sets of source vertices per mesh, each
 * source with a start offset, per set and vertex the shortest distance along the mesh graph, the predecessor on a shortest path and
 * the source the path starts from (trimesh's `vertex_adjacency_graph` with a networkx shortest path), and one info record per (mesh,
 * set).  Everything is float64, operation by operation; corners are widened from the resident "verts" as sh_mass_properties widens
 * them; indices are local to the mesh; "degenerate" and "row" mean what they mean in sh_mesh_topology; dot3(a, b) = (a0 b0 + a1 b1) +
 * a2 b2.  Nothing is transcendental: the result is the same bytes wherever the rule runs.
 *   face record  "geo.face", 6 doubles per face at 6 foff[b]: len[3], unf[3].  Slot e concerns the edge {f[e], f[(e + 1) % 3]}, as in
 *                "topo.adj".  len[e]: with lo = min and hi = max of the two indices and D = P_hi - P_lo, len[e] = sqrt(dot3(D, D)); the
 *                canonical order makes both faces of an edge store the same bytes.  unf[e] is the length of the straight line between
 *                the two vertices opposite the edge with the two faces unfolded into one plane, +inf unless g = adj[f][e] >= 0.  With a, b
 *                the edge, p the third vertex of f and q the vertex of g that is neither a nor b: lo / hi = min / max(a, b), p' = min(p,
 *                q), q' = max(p, q); E = P_hi - P_lo, l = sqrt(dot3(E, E)); for r in {p', q'}: d_r = P_r - P_lo, x_r = dot3(d_r, E) / l,
 *                t = dot3(d_r, d_r) - x_r * x_r, y_r = sqrt(t < 0 ? 0 : t); s = y_p' + y_q', x_c = (x_p' * y_q' + x_q' * y_p') / s,
 *                dx = x_p' - x_q', unf = sqrt(dx * dx + s * s).  It is valid only if p != q, s > 0, x_c > 0 and x_c < l -- the line
 *                crosses the open shared edge; comparisons are false on NaN -- and +inf otherwise.  A degenerate face has six +inf.
 *   graph        vertex v has one arc per non-degenerate face f of its row and per corner k with f[k] == v: to f[(k + 1) % 3] with
 *                len[k]; to f[(k + 2) % 3] with len[(k + 2) % 3]; with SH_GEO_UNFOLD also to the vertex opposite slot (k + 1) % 3 with
 *                unf[(k + 1) % 3].  Parallel arcs are harmless: the minimum takes one.  SH_GEO_EDGES is the vertex adjacency graph of
 *                trimesh; SH_GEO_UNFOLD adds the unfolded diagonals.  Every arc has its reverse with the same bytes.
 *   distance     set k of mesh b is a list of (vertex, d0) pairs, d0 >= 0 and finite.  d[v] is the minimum, over the listed pairs and all
 *                arc paths from them, of the left fold fl(fl(d0 + w1) + w2) ...; a value above max_dist (+inf, or > 0) counts as +inf,
 *                and a candidate that is not finite is ignored.  fl(a + w) is monotone in a and never below a, so this minimum is the
 *                unique fixed point of d[v] = min(d0s of v, min over arcs u -> v of fl(d[u] + w)): ANY relaxation schedule run until
 *                nothing changes gives the same bytes, and so does Dijkstra; a prefix of a path within max_dist is within it, so the
 *                cut-off changes no kept value.  THEREFORE NO SCHEDULE IS PART OF THIS DEFINITION; `sweeps` of the info record says
 *                how many rounds the library took, is informational and is to be compared with nothing.  The distance is symmetric
 *                between two vertices up to rounding, not as bytes (the fold runs from the source).
 *   roots, predecessors, sources   from the converged d alone.  v is a root when a listed d0 of v equals d[v]; its label is the
 *                smallest position in the set's list with that d0.  Otherwise pred[v] is the smallest u with an arc u -> v, fl(d[u] + w)
 *                == d[v] and d[u] < d[v].  pred[v] is SH_GEO_ROOT at a root, SH_GEO_UNREACHED when d[v] is +inf, and SH_GEO_NO_PRED when
 *                v is reached but no such u exists: that happens only behind an arc of length 0 (two vertices at the same coordinates
 *                joined by a face) or one that d[u] absorbs (fl(d[u] + w) == d[u]).  d falls strictly along pred, so the predecessors
 *                form a forest.  source[v] is the label of the root of v's tree, -1 when v is unreached or its chain ends in SH_GEO_NO_PRED.
 *   info         per (b, k) SH_GEO_INFO_BYTES = 32 bytes: double far_dist, the largest finite d (0.0 when none); int32 reached, roots,
 *                no_pred, farthest (the vertex of far_dist, the smallest index among equals, -1 when none), sweeps, status (0).  The
 *                layout is stated here and by shoulder_amd._lib.GEO_INFO_DTYPE; it is not a typedef of this header.
 *
 * Arguments in this order: the context (SH_ERR_ARG); mode SH_GEO_EDGES or SH_GEO_UNFOLD, K in 1..SH_GEO_MAX_SETS, max_dist +inf or > 0
 * (SH_ERR_ARG); the lists: src_off (B K + 1 int32, ascending from 0; set k of mesh b is [src_off[b K + k], src_off[b K + k + 1])), src,
 * d0 (null: zeros) -- every source index in [0, V_b), every d0 finite and >= 0, checked on the host before anything is enqueued
 * (SH_ERR_ARG with the offending mesh, set and position in the text; without a resident batch there is no set to read and the state
 * answers).  An empty set is allowed: nothing is reached.  Then a resident batch and no runs in flight (SH_ERR_STATE); the incidence of
 * THIS batch resident (SH_ERR_STATE: call sh_mesh_topology first; a topology that ran out of rounds is accepted); SH_ERR_NOMEM when the
 * buffers do not fit.  A (mesh, set) pair with V_b <= SH_GEO_LDS_VERTICES is relaxed by one workgroup with its distances in LDS; a
 * larger mesh takes Jacobi rounds on two planes in memory, SH_GEO_CHUNK rounds between two looks of the host at one 4-byte word, at
 * most max V_b + 1 rounds, which the rule cannot exceed: beyond them SH_ERR_INTERNAL.  Reads "verts", "faces", the offsets, "topo.vrow",
 * "topo.vface", "topo.adj".  Resident afterwards: "geo.face"; "geo.dist", per mesh K planes of V_b doubles at K voff[b] + k V_b;
 * "geo.pred" and "geo.source", int32 in the same places; "geo.info", B K records; and the scratch "geo.opp", "geo.plane", "geo.jump",
 * "geo.src", "geo.d0", "geo.state".  They are removed together with "topo.*" by the next upload / commit / sh_store("verts").  Every
 * other buffer keeps its bytes. */
#define SH_GEO_EDGES        0
#define SH_GEO_UNFOLD       1
#define SH_GEO_MAX_SETS     16
#define SH_GEO_LDS_VERTICES 20000      /* 160 000 B of distances; 3 840 B of the 163 840 B of LDS stay for flags */
#define SH_GEO_CHUNK        32         /* rounds of the general path between two looks of the host */
#define SH_GEO_INFO_BYTES   32
#define SH_GEO_ROOT         (-1)
#define SH_GEO_NO_PRED      (-2)
#define SH_GEO_UNREACHED    (-3)
int sh_geodesic(sh_ctx*, int mode, int K, double max_dist, const int32_t* src_off /* B K + 1, host */, const int32_t* src /* host */,
                const double* d0 /* host, nullable */, double* dist /* K sumV, host, nullable */, int32_t* pred /* K sumV, host, nullable */,
                int32_t* source /* K sumV, host, nullable */, void* info /* B K x SH_GEO_INFO_BYTES, host, nullable */);

/* ---- smoothing of the vertices of the resident batch ----------------------------------------------------------------------------------------
 * Surfaces segmented from CT carry the voxel staircase; this moves the vertices themselves (k_smooth.h): the vertex -> vertex rows of
 * every mesh (trimesh's `vertex_neighbors`) and on them the Laplacian, Taubin and HC filters (trimesh.smoothing.filter_laplacian,
 * filter_taubin, filter_humphrey).  Everything is float64, operation by operation, + - x / sqrt only; indices are local to the mesh;
 * "degenerate" and "row" mean what they mean in sh_mesh_topology; dot3(a, b) = (a0 b0 + a1 b1) + a2 b2.  The result is the same bytes
 * wherever the rule runs, and a mesh's result depends on that mesh and the arguments alone: not on B, its place in the batch or a launch.
 *   start        P0 is the resident float32 "verts" widened to float64.
 *   rows         "smooth.nrow", int32, V_b + 1 entries per mesh at voff[b] + b, exclusive prefix sums; "smooth.nbr", int32, mesh b from
 *                6 foff[b] (room for two neighbours per corner; the mesh uses the first nrow[V_b] places): row v lists the DISTINCT
 *                vertices u != v that share a non-degenerate face with v in ASCENDING index -- the order is part of the definition: it
 *                is the order of every sum below.  As sets the rows are trimesh's vertex_neighbors on a mesh without degenerate faces.  A
 *                vertex no face uses has an empty row; a row has no assumed length.  The rows depend on the faces alone, are built once
 *                and stay resident for the batch.
 *   weights      SH_SMOOTH_UNIFORM: w = 1.0 for every neighbour.  SH_SMOOTH_INVLEN: w_vu = 1.0 / l, l = sqrt(dot3(D, D)), D = P0_hi - P0_lo
 *                with lo = min(v, u), hi = max(v, u): both directions hold the same bytes, as "geo.face" does.  They are taken ONCE, from
 *                P0, and kept in "smooth.w" beside "smooth.nbr" (float64, the same places); a neighbour with l == 0.0 or l not finite is
 *                stored as 0.0 and skipped under SH_SMOOTH_INVLEN: it enters neither sum.
 *   mean         M(x)[v] of a field x of 3 doubles per vertex: S = sum w x[u], W = sum w, the accumulators starting at 0.0 and adding one
 *                term per neighbour in the row's order, component by component (each term the product w * x[u][c], then the sum);
 *                M(x)[v] = S / W.  M(x)[v] = x[v] instead when v is pinned, the row is empty, nothing was added or W is not finite.
 *   step         step(P, c)[v] = P[v] + c * (M(P)[v] - P[v]): the difference, then the product, then the sum.
 *   filters      all iterate from P = P0; with 0 iterations the result is P0 and the call only builds the rows.
 *                SH_SMOOTH_LAPLACIAN (p0 = lambda): iterations x step(., lambda).
 *                SH_SMOOTH_TAUBIN (p0 = lambda, p1 = mu <= 0): an iteration is step(., lambda), then step(., mu).
 *                SH_SMOOTH_HC (p0 = alpha, p1 = beta; Vollmer's Humphrey's-classes filter), per iteration: q = P; p = M(q);
 *                b = p - (alpha * P0 + (1.0 - alpha) * q), the bracket added left to right; P = p - (beta * b + (1.0 - beta) * M(b)),
 *                M(b) with the same rows, weights and pins.  At a pinned vertex b is 0.0 by definition (alpha x + (1 - alpha) x need not
 *                round to x), so p = q = P0 there and it stays put.
 *   pins         a vertex is pinned when its byte of the optional host mask `pin` (sumV bytes) is non-zero, or when SH_SMOOTH_PIN_BORDER
 *                is set and one of the two slots of "topo.adj" that touch it in a face of its incidence row is SH_ADJ_BORDER or
 *                SH_ADJ_NONMANIFOLD: the test behind SH_VERT_BORDER | SH_VERT_NONMANIFOLD.
 *   keep volume  SH_SMOOTH_KEEP_VOLUME: after the last iteration one uniform scaling about the centre of mass restores the volume of P0.
 *                With T(X) the sums of terms 13 .. 16 of sh_mass_properties (d = dot3(a, cross3(b, c)) and d s, the pivot o = P0 of
 *                vertex 0 for both) over ALL faces of the mesh on the vertices X, in THE TREE of that call (blocks of SH_MASS_BLOCK faces,
 *                h = 128 .. 1, the block sums in block order): V0 = T13(P0) / 6.0, V1 = T13(P) / 6.0, c = T14..16(P) / (4.0 * T13(P)) + o,
 *                r = V0 / V1, s ten Newton steps from s = 1.0 on s^3 = r, each s = s - ((s * s) * s - r) / (3.0 * (s * s));
 *                P[v] = c + s * (P[v] - c).  A mesh gets status SH_ERR_GEOMETRY and NO scaling when V0 or V1 is 0.0 or not finite, r lies
 *                outside [1/8, 8] or c is not finite -- never the batch.  The flag together with a pin (a mask pointer or
 *                SH_SMOOTH_PIN_BORDER) is SH_ERR_ARG: a scaling moves pinned vertices.  In exact arithmetic the filters commute with a
 *                uniform scaling, so one scaling at the end is what trimesh's per-iteration `volume_constraint` amounts to; equality with
 *                trimesh is not claimed.
 *   info         per mesh SH_SMOOTH_INFO_BYTES = 64 bytes, resident in "smooth.info": double volume_before (V0), volume_after (V1: before
 *                the scaling), scale (s; 1.0 without the flag or with the status), max_disp, sum_sq_disp; int32 pinned, isolated (empty
 *                rows), status, and three int32 of padding (0).  max_disp is the largest |P - P0| = sqrt(dot3(d, d)) of the result, a
 *                value that is no number counting as 0.0; sum_sq_disp is the sum of dot3(d, d) over blocks of 256 consecutive vertices
 *                in the same tree shape.  The layout is stated here and by shoulder_amd._lib.SMOOTH_INFO_DTYPE; it is not a typedef.
 *
 * Arguments in this order: the context (SH_ERR_ARG); filter, weight, iterations in 0..SH_SMOOTH_MAX_ITER and flags with known bits
 * (SH_ERR_ARG); the two parameters, both finite whatever the filter, lambda in [0, 1], mu in [-1, 0], alpha and beta in [0, 1] (SH_ERR_ARG,
 * the text names the argument; p1 of SH_SMOOTH_LAPLACIAN is not used); SH_SMOOTH_KEEP_VOLUME with a pin (SH_ERR_ARG); a resident batch
 * and no runs in flight (SH_ERR_STATE); the incidence of THIS batch resident (SH_ERR_STATE: call sh_mesh_topology first; a topology
 * that ran out of rounds is accepted).  SH_ERR_NOMEM when the buffers do not fit, or when the largest mesh has more than (2^31 - 1) / 6
 * faces (its row starts are int32 and it has six places for neighbours per face).  The host enqueues every launch of the call (their
 * number follows from the arguments: 3 for the rows when they are not resident, 1 + the M(.) evaluations + 5) and looks at nothing in
 * between.  out (sumV x 3 doubles) and info may be NULL.  Reads "verts", "faces", the offsets, "topo.vrow", "topo.vface", "topo.adj";
 * does NOT write "verts".  Resident afterwards: "smooth.pos" (3 doubles per vertex at 3 voff[b]), "smooth.nrow", "smooth.nbr",
 * "smooth.w", "smooth.info" and the scratch "smooth.plane" (three planes: two of the iteration, one for b), "smooth.pin", "smooth.mask",
 * "smooth.part".  They are removed together with "topo.*" by the next upload / commit / sh_store("verts").  Every other buffer keeps
 * its bytes. */
#define SH_SMOOTH_LAPLACIAN   0
#define SH_SMOOTH_TAUBIN      1
#define SH_SMOOTH_HC          2
#define SH_SMOOTH_UNIFORM     0
#define SH_SMOOTH_INVLEN      1
#define SH_SMOOTH_PIN_BORDER  1
#define SH_SMOOTH_KEEP_VOLUME 2
#define SH_SMOOTH_MAX_ITER    256
#define SH_SMOOTH_INFO_BYTES  64
int sh_smooth_vertices(sh_ctx*, int filter, int weight, int iterations, int flags, double p0, double p1,
                       const unsigned char* pin /* sumV, host, nullable */, double* out /* sumV x 3, host, nullable */,
                       void* info /* B x SH_SMOOTH_INFO_BYTES, host, nullable */);

/* ---- repair of the resident batch: one winding, outward shells, filled holes ----------------------------------------------------------
 * sh_mesh_topology counts what is wrong with a mesh; this puts it right (k_repair.h), as trimesh.repair's fix_winding, fix_inversion and
 * fill_holes do, for holes of any length.  "verts" and "faces" are NOT written: the repaired meshes come back in "repair.faces" and
 * "repair.verts", ready for an upload.  Every rule is per mesh with indices local to the mesh; "degenerate", "slot", "shell" and
 * same(f, g) ("both faces traverse the edge in the same direction") mean what they mean in sh_mesh_topology; a result depends on the
 * mesh and the options alone: not on B, the mesh's place in the batch or a schedule.  dot3(a, b) = (a0 b0 + a1 b1) + a2 b2, float64,
 * no contraction.
 *   winding      (orient >= SH_REPAIR_WINDING) per shell with first face r: parity(r) = 0 and, across every slot >= 0, parity(g) =
 *                parity(f) XOR same(f, g).  The parities are unique exactly when the shell is orientable, so any schedule gives them: one
 *                workgroup per mesh walks the face graph breadth first from all first faces at once, the state in LDS.  A shell in which
 *                a manifold slot contradicts the parities is SH_REPAIR_NONORIENTABLE: no face of it is flipped, none of its holes is
 *                filled and no parity of it is reported.  A face of parity 1 is flipped: (a, b, c) becomes (a, c, b), which exchanges its
 *                slots 0 and 2.  Degenerate faces are copied and never flipped.  A mesh with more than SH_REPAIR_LDS_FACES faces, or whose
 *                walk is deeper than max_rounds levels, gets status SH_ERR_CAPACITY and an unchanged copy, as does a mesh whose
 *                topology did not finish -- never the batch.
 *   outward      (orient >= SH_REPAIR_OUTWARD) per orientable shell among the shells_written of the topology: V6 = the sum of
 *                det[A - o, B - o, C - o] = dot3(a, cross3(b, c)) over its parity-corrected faces, the float32 corners widened, o the
 *                centre of the shell's box in "topo.shells", lo + (hi - lo) * 0.5 per coordinate in float64.  The order: the shell's
 *                faces ascending, in blocks of 2 048 consecutive entries of that list; one after the other inside a block from 0.0, then
 *                the block sums one after the other from 0.0.  V6 < 0: the shell is inverted and all its faces are flipped once more;
 *                V6 == 0: nothing.  Shells behind shells_written get their winding alone, and bit 1 of the mesh's flags says so.
 *   nested       (orient == SH_REPAIR_NESTED) every written shell is made outward as above; then for shell k, with p_k the first
 *                corner of its first face, W_k = (the sum of solid_angle_tri(p_k, .) over the outward faces of all OTHER written shells
 *                that are orientable and closed: no border slot, no non-manifold slot) / (4 pi), summed in the block order of
 *                sh_winding_numbers over the mesh's face indices, the excluded faces skipped.  depth = rint(W_k); a shell of odd depth
 *                is flipped inward; |W_k - depth| > 0.25: shell status SH_REPAIR_AMBIGUOUS and depth 0.  A mesh with more shells than
 *                shells_written gets SH_ERR_CAPACITY and is treated as SH_REPAIR_OUTWARD.
 *   holes        traced on the ORIENTED faces, after all flips.  A border half-edge is a (face f, slot e) whose adjacency is
 *                SH_ADJ_BORDER; it runs from f[e] to f[(e + 1) % 3] and has the id 3 f + e.  Its successor: rotate about the head w;
 *                slot (e + 1) % 3 of f starts at w; a border there is the successor; a face g there is entered through its slot that
 *                runs the other way and the rotation goes on from that slot; SH_ADJ_NONMANIFOLD there, or a g that runs the same way
 *                (only in a shell that is not orientable), blocks the chain.  The successor is injective, so the border half-edges fall
 *                into cycles and blocked chains.  The half-edges of blocked chains are only counted (blocked_edges).  Where two holes
 *                touch in a vertex the rotation leads from one into the other, so a cycle that passes a vertex more than once is CUT
 *                there: each of its half-edges with that head takes the successor of the one with the same head before it along
 *                the cycle (cyclically), which closes every stretch between two passes into a cycle of its own; half-edges of
 *                different cycles (two sheets that touch in a vertex) are left alone.  The cut is made once.  A cycle is then a
 *                hole: its start is its smallest id, its length L its edges; the holes of a mesh are ordered by start.  All of it is
 *                found by pointer doubling over the compacted border half-edges, in a number of rounds fixed by their count.
 *   fill         a hole is filled when its shell is orientable and 3 <= L <= max_hole_edges; else its status says why.  With the
 *                tails u_0 (the start's), u_1, ... in successor order: SH_REPAIR_FAN adds the faces (u_0, u_{j+1}, u_j), j = 1 .. L - 2,
 *                and no vertex; SH_REPAIR_CENTROID one vertex c and the faces (u_{j+1}, u_j, c), j = 0 .. L - 1, indices mod L, c per
 *                coordinate the float64 sum of the float32 positions from u_0 in loop order, over (double) L, rounded once to float32;
 *                SH_REPAIR_FILL_NONE reports the holes only.  New faces follow the mesh's own in hole order and in j order within a
 *                hole; new vertices follow the mesh's in hole order.
 *   records      sh_repair_info per mesh ("repair.info"): status; shells_nonorientable; shells_inverted; faces_flipped (final); holes
 *                (exact whatever max_holes); holes_written; holes_filled; largest_hole (edges); blocked_edges; faces_added; verts_added;
 *                faces_out; verts_out; flags (bit 0: anything changed, bit 1: shells behind shells_written were not made outward);
 *                shell_records = the records per mesh of "repair.shells" (the max_shells of the topology); reserved.
 *                sh_repair_shell per written shell ("repair.shells"): status 0, SH_REPAIR_NONORIENTABLE or SH_REPAIR_AMBIGUOUS;
 *                parity_flips; inverted; depth (-1 when not asked); holes; holes_filled; V6; W.
 *                sh_repair_hole for the first max_holes holes per mesh ("repair.holes"): shell; start_face; start_slot (of the oriented
 *                face); edges; status SH_REPAIR_HOLE_*; first_face in the output, or -1; faces_added; vertex, or -1.
 *   buffers      "repair.flip", uint8 per face at foff[b]: the final flip.  "repair.off", int64, 3 (B + 1): the starts of the meshes in
 *                "repair.faces" (in faces), in "repair.verts" (in vertices) and in the border scratch; the host sizes them before the
 *                first launch from "topo.info": F_b + border_edges faces and V_b + border_edges / 3 vertices per mesh, of which
 *                faces_out and verts_out are used.
 * Arguments in this order: the context and options (SH_ERR_ARG); orient in 0..3, fill in 0..2, max_hole_edges >= 3, max_holes in
 * 1..SH_REPAIR_MAX_HOLES, max_rounds in 1..SH_REPAIR_MAX_ROUNDS, reserved == 0 (SH_ERR_ARG); a resident batch and no runs in flight
 * (SH_ERR_STATE); the topology of THIS batch resident (SH_ERR_STATE: call sh_mesh_topology first).  SH_ERR_NOMEM when the buffers do not
 * fit.  The host reads "topo.info" once, enqueues a fixed list of launches and looks at nothing in between.  Every output pointer may
 * be NULL.  Reads "verts", "faces", the offsets, "topo.adj", "topo.label", "topo.vrow", "topo.vface", "topo.info", "topo.shells".  Resident afterwards: "repair.flip",
 * "repair.faces", "repair.verts", "repair.info", "repair.shells", "repair.holes", "repair.off" and the scratch "repair.par", "repair.work",
 * "repair.edge", "repair.term"; they are removed together with "topo.*" by the next upload / commit / sh_store("verts").  Every other
 * buffer keeps its bytes. */
#define SH_REPAIR_NONE            0
#define SH_REPAIR_WINDING         1
#define SH_REPAIR_OUTWARD         2
#define SH_REPAIR_NESTED          3
#define SH_REPAIR_FILL_NONE       0
#define SH_REPAIR_FAN             1
#define SH_REPAIR_CENTROID        2
#define SH_REPAIR_NONORIENTABLE   1
#define SH_REPAIR_AMBIGUOUS       2
#define SH_REPAIR_HOLE_FILLED     0
#define SH_REPAIR_HOLE_TOO_LONG   1
#define SH_REPAIR_HOLE_SHELL      2
#define SH_REPAIR_HOLE_OPEN       3
#define SH_REPAIR_HOLE_TOO_SHORT  4
#define SH_REPAIR_MAX_HOLES       65536
#define SH_REPAIR_MAX_ROUNDS      1048576
#define SH_REPAIR_LDS_FACES       131072
#define SH_REPAIR_CHANGED         1
#define SH_REPAIR_SHELLS_LEFT     2
struct sh_repair_options { int32_t orient, fill, max_hole_edges, max_holes, max_rounds, reserved; };            /* 24 B */
typedef struct sh_repair_options sh_repair_options;
struct sh_repair_info {
  int32_t status, shells_nonorientable, shells_inverted, faces_flipped, holes, holes_written, holes_filled, largest_hole;
  int32_t blocked_edges, faces_added, verts_added, faces_out, verts_out, flags, shell_records, reserved;
};                                                                                                             /* 64 B */
typedef struct sh_repair_info sh_repair_info;
struct sh_repair_shell { int32_t status, parity_flips, inverted, depth, holes, holes_filled; double V6, W; };   /* 40 B */
typedef struct sh_repair_shell sh_repair_shell;
struct sh_repair_hole { int32_t shell, start_face, start_slot, edges, status, first_face, faces_added, vertex; }; /* 32 B */
typedef struct sh_repair_hole sh_repair_hole;
int sh_mesh_repair(sh_ctx*, const sh_repair_options* options, sh_repair_info* info /* B, host, nullable */,
                   sh_repair_shell* shells /* B x shell_records, host, nullable */, sh_repair_hole* holes /* B x max_holes, host, nullable */,
                   unsigned char* flip /* sumF, host, nullable */);

/* ---- simplification of the resident batch: vertex clustering with quadric placement -------------------------------------------------
 * sh_mesh_simplify makes every resident mesh smaller (k_simplify.h): the used vertices that fall into one cell of a grid become one
 * vertex, placed at their mean or where the quadric of their faces is smallest, and the faces that survive are renumbered
 * (Rossignac-Borrel clustering with Garland-Heckbert quadrics, as in Lindstrom's out-of-core simplification).  The placement is
 * Lindstrom's cell clamp with a Tikhonov term towards the mean in place of his SVD; equality with any other library is not claimed.
 * "verts" and "faces" are NOT written: the meshes come back in "simp.verts" and "simp.faces", ready for an upload.  Clustering does
 * not preserve topology: it may leave border and non-manifold edges, which sh_mesh_topology of the re-upload reports.  Every rule is
 * per mesh with indices local to the mesh, float64 operation by operation with + - x / sqrt and floor only, no contraction, dot3(a, b) =
 * (a0 b0 + a1 b1) + a2 b2, cross3(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); "degenerate" and "row" mean what they mean in
 * sh_mesh_topology; a result depends on the mesh, its cell and the options alone: not on B, the mesh's place in the batch or a
 * schedule.  The rules are sh_scalar.h simp_*, restated by tests/simplify_oracle.py.
 *   used       a vertex is used when a non-degenerate face names it (its row is not empty).  An unused vertex takes no part in
 *              anything; its map entry is -1.
 *   grid       lo, hi: the float32 minima and maxima of the used vertices, widened; h = cell[b]; per axis n = (int64) floor((hi - lo) / h)
 *              + 1; the cell of a vertex per axis i = min((int64) floor(((double) x - lo) / h), n - 1); key = (iz ny + iy) nx + ix.  A
 *              mesh with n > SH_SIMPLIFY_MAX_CELLS on an axis, or with more than SH_SIMPLIFY_MAX_CLUSTERS clusters, gets status
 *              SH_ERR_CAPACITY, empty outputs, a map of -1 and, of the counts, verts_used and clusters (0 for the axis limit) alone --
 *              never the batch.
 *   clusters   a cluster is the set of used vertices with one key; clusters are numbered ascending by key; the members of a cluster
 *              are taken ascending by vertex index (part of the definition: the sums below run in that order); o = lo + ((double) i +
 *              0.5) h per axis, the centre of the cell.
 *   mean       m = S / (double) count, S the sum of the widened positions, one member after the other, from 0.0.
 *   quadric    of a vertex, relative to the o of its cluster: over its row in row order, from 0.0, each face with the widened corners
 *              A, B, C adds n = cross3(B - A, C - A) and d = -dot3(n, A - o) to the ten sums n0n0, n0n1, n0n2, n1n1, n1n2, n2n2, n0d,
 *              n1d, n2d, dd.  n is not normalised: a face weighs by its squared area; a face with two corners in a cluster counts
 *              twice, as Garland-Heckbert's Q1 + Q2 does.  Of a cluster: the quadrics of its members added in member order from 0.0.
 *              With A the 3 x 3 matrix (a00 a01 a02; . a11 a12; . . a22) of the first six sums and b the next three:
 *   place      SH_SIMPLIFY_MEAN: float32(m).  SH_SIMPLIFY_QUADRIC: tr = (a00 + a11) + a22, lam = reg tr, m00 = a00 + lam, m11 = a11 +
 *              lam, m22 = a22 + lam, r = lam (m - o) - b per axis, then term by term
 *                l00 = sqrt(m00); l10 = a01 / l00; l20 = a02 / l00; p1 = m11 - l10 l10; l11 = sqrt(p1); l21 = (a12 - l20 l10) / l11;
 *                p2 = (m22 - l20 l20) - l21 l21; l22 = sqrt(p2); y0 = r0 / l00; y1 = (r1 - l10 y0) / l11;
 *                y2 = ((r2 - l20 y0) - l21 y1) / l22; x2 = y2 / l22; x1 = (y1 - l21 x2) / l11; x0 = ((y0 - l10 x1) - l20 x2) / l00
 *              and the position is float32(o + x).  The cluster takes float32(m) instead, and counts in fallbacks, when tr is 0.0 or
 *              not finite, a radicand (m00, p1, p2) is <= 0.0 or not finite, a component of x is not finite, or |x_c| > (0.5 h) clamp.
 *   faces      a non-degenerate face (a, b, c) becomes (c(a), c(b), c(c)), its winding kept; it is COLLAPSED and dropped when two of
 *              the three are equal; of the rest, those with the same set of three clusters are DUPLICATES and the one with the
 *              smallest face index stays; kept faces keep the order of their indices.  Clusters no kept face names are dropped and
 *              the rest renumbered in key order: the output has no unreferenced vertex.  map[v] = the output vertex of v's cluster,
 *              or -1.
 *   outputs    the regions of mesh b start at voff[b] (in "simp.verts" and "simp.map") and foff[b] (in "simp.faces"); an output is
 *              never larger than its input, so the host sizes nothing from the device and reads nothing between the launches.  The
 *              tail of a region behind verts_out / faces_out is zero.
 *   records    sh_simplify_info per mesh ("simp.info"): status (0, SH_ERR_CAPACITY, or SH_ERR_GEOMETRY with faces_out = 0 when every
 *              face collapsed or the mesh has no used vertex); verts_used; clusters; verts_out; faces_out; faces_collapsed;
 *              faces_duplicate (the dropped ones); fallbacks; largest_cluster (members); reserved 0; cell = cell[b]; max_move = the
 *              largest sqrt(dot3(d, d)), d = a used vertex (widened) minus its cluster's float32 position (widened), 0.0 for a d that
 *              gives no number; 8 bytes of 0.
 * Arguments in this order: the context and options (SH_ERR_ARG); place SH_SIMPLIFY_MEAN or SH_SIMPLIFY_QUADRIC, reserved == 0, reg
 * finite in [0, 1], clamp finite and > 0 (SH_ERR_ARG); a cell array, every cell[b] of the resident meshes finite and > 0 (SH_ERR_ARG,
 * naming b); a resident batch and no runs in flight (SH_ERR_STATE); the incidence of THIS
 * batch resident (SH_ERR_STATE: call sh_mesh_topology first); SH_ERR_NOMEM when the buffers do not fit or the batch has more than
 * 2^31 - 1 vertices.  A fixed list of launches; every output pointer may be NULL.  Reads "verts", "faces", the offsets, "topo.vrow",
 * "topo.vface".  Resident afterwards: "simp.verts" (float32, 3 sumV), "simp.faces" (int32, 3 sumF), "simp.map" (int32, sumV),
 * "simp.info" and the scratch "simp.state", "simp.seg", "simp.cell", "simp.key", "simp.sorted", "simp.ukey", "simp.start", "simp.cid",
 * "simp.mark", "simp.rank", "simp.quad", "simp.pos", "simp.keep", "simp.frank", "simp.tmp"; they are removed together with "topo.*" by
 * the next upload / commit / sh_store("verts").  Every other buffer keeps its bytes. */
#define SH_SIMPLIFY_MEAN          0
#define SH_SIMPLIFY_QUADRIC       1
#define SH_SIMPLIFY_MAX_CELLS     1048576
#define SH_SIMPLIFY_MAX_CLUSTERS  2097152
struct sh_simplify_options { int32_t place, reserved; double reg, clamp; };                                     /* 24 B */
typedef struct sh_simplify_options sh_simplify_options;
struct sh_simplify_info {
  int32_t status, verts_used, clusters, verts_out, faces_out, faces_collapsed, faces_duplicate, fallbacks, largest_cluster, reserved;
  double cell, max_move;
  int32_t pad[2];
};                                                                                                             /* 64 B */
typedef struct sh_simplify_info sh_simplify_info;
int sh_mesh_simplify(sh_ctx*, const sh_simplify_options* options, const double* cell /* B, host */, sh_simplify_info* info /* B, host, nullable */,
                     float* verts /* sumV x 3, host, nullable */, int32_t* faces /* sumF x 3, host, nullable */, int32_t* map /* sumV, host, nullable */);

/* ---- a face hierarchy of the resident batch, and the closest-point step through it -------------------------------------------------
 * sh_mesh_bvh builds, per resident mesh, a bounding-box hierarchy over its faces (k_bvh.h; the rules are sh_scalar.h bvh_*, all float32
 * min / max, one float64 quantisation and integer work, restated by tests/bvh_oracle.py):
 *   loose     a face with !(g >= 2^-7), g = |ab x ac|^2 / Lmax^3 (bvh_loose: slivers, collinear and point triangles, the faces the cull of
 *             sh_closest_points never skips) stays out of the tree: "bvh.loose" lists them ascending by face id, every query tests all.
 *   order     the other ("tight") faces ascending by (code, face id), code the 30-bit interleave of the box centre quantised to 1024
 *             cells per axis of the box of the tight faces (bvh_quant, bvh_code): "bvh.order".  "bvh.tri" holds their corners in that
 *             order, 9 float32 each.
 *   tree      implicit, no child pointers: a leaf is SH_BVH_LEAF consecutive entries of the order (the last may be short), node j of
 *             level k + 1 covers the nodes [j W, (j + 1) W) of level k that exist, W = SH_BVH_WIDTH, until a level has one node.  A node
 *             is its box, 6 float32 (lo, hi; minima and maxima in the order of bvh_fmin / bvh_fmax, -0 below +0): "bvh.box", the levels of
 *             a mesh one after the other, mesh b at the node "bvh.off"[b][5].  A mesh without tight faces has no levels.
 *   "bvh.off" per mesh 32 int32: tight, loose, leaves, levels, nodes, the mesh's first node in "bvh.box", 0, 0, then the first node of
 *             each level relative to that and, behind the last level, nodes again.  The first node of a mesh is the sum of the nodes a
 *             mesh of F_a tight faces would have over the meshes a before it: it depends on the face COUNTS before it, nothing else does.
 *   sh_bvh_info (48 B, all int32 / float32) per mesh, resident in "bvh.info": tight, loose, leaves, levels, nodes, reserved = 0, and the
 *             box of the tight faces lo[3], hi[3] (zeros without one).
 * Arguments in this order: the context (SH_ERR_ARG); a resident batch and no runs in flight (SH_ERR_STATE; a run is not needed).
 * SH_ERR_NOMEM when the buffers do not fit.  "bvh.order" and "bvh.loose" have F_b int32 per mesh at foff[b], the unused tail -1.  The
 * "bvh.*" buffers answer for the batch they were built for: the next upload / commit / sh_store("verts") removes them.  The call
 * changes nothing else: every other named buffer keeps its bytes.
 *
 * sh_set_query_accel(SH_ACCEL_BVH) routes the closest-point step of sh_closest_points, sh_register_points and sh_register_multistart
 * through the hierarchy (k_cp_tree instead of k_cp_walk; the index is built first when "bvh.order" is not resident).  A node is skipped
 * only when every face in it would compute a d2 strictly above the point's best (k_bvh.h states the argument), and the winner is the
 * minimum of (d2, face) under a total order: THE RESULTS ARE THE SAME BYTES in either mode.  SH_ACCEL_OFF (0) is the default; a mode
 * that is neither is SH_ERR_ARG.  The same switch routes sh_ray_cast and sh_ray_nearest through the hierarchy (see the rays above; the
 * box-frame rays of sh_anp_axis_hits stay on the walk over all faces).  sh_winding_numbers, the samples and the geodesics do not read the
 * index. */
#define SH_ACCEL_OFF      0
#define SH_ACCEL_BVH      1
#define SH_BVH_INFO_BYTES 48
struct sh_bvh_info { int32_t tight, loose, leaves, levels, nodes, reserved; float lo[3], hi[3]; };             /* 48 B */
typedef struct sh_bvh_info sh_bvh_info;
int sh_mesh_bvh(sh_ctx*, sh_bvh_info* out /* B, host, nullable */);
int sh_set_query_accel(sh_ctx*, int mode);
int sh_get_query_accel(const sh_ctx*);

/* ---- stage-level access for parity tests: named intermediate device buffers ----------
 * names: "verts_obb" "obb_transform" "full.zs" "full.centroids" "full.areas" "full.nloops"
 * "distal.*" "prox.*" "prox.ixy" "prox.itr_start" "prox.itr_centered_start" "canal.points"
 * "groove.X" "groove.nX" "groove.proba" "anp.image" "anp.logits" "anp.roll" ... (see sh_buffer_info) */
int  sh_buffer_info(sh_ctx*, const char* name, size_t* nbytes, int* elem_size);
/* Device address of a named buffer (e.g. "verts_obb", "verts_csys": inputs / outputs of sh_affine_apply; valid until the
 * next upload). */
int  sh_buffer_device(sh_ctx*, const char* name, void** dev_ptr, size_t* nbytes);
int  sh_fetch(sh_ctx*, const char* name, void* host, size_t nbytes);
int  sh_store(sh_ctx*, const char* name, const void* host, size_t nbytes);

/* The anatomic-neck network alone (replaces the `onnxruntime.InferenceSession.run` call of
 * humerus/anatomic_neck.py:67-76): n images [n][H][W] float32 (host) -> logits [n][H][W] float32
 * (host), computed in sh_params.unet_dtype.  H and W must be multiples of 16 << depth. */
int  sh_unet_infer(sh_ctx*, const float* images, int n, int H, int W, float* logits);

/* Average duration (ms) of the named kernel over the launches since the last reset, measured
 * with HIP events on the ctx stream (bench.py roofline); name NULL resets all timers. */
int  sh_kernel_time_ms(sh_ctx*, const char* kernel, double* avg_ms, int* launches);
/* level 0: off; 1: events around every launch; 2: around the UNet layers only (events around all ~150 launches of a
 * run stretch it by ~4 % at B = 64, so a measurement inside a timed region uses level 2). */
int  sh_enable_timing(sh_ctx*, int level);

/* Streaming use (one sh_run after another on the resident batch): with overlap on, sh_run starts a
 * background thread, once all its device work is enqueued, that computes the convex hulls the NEXT
 * sh_run(SH_STAGE_OBB) needs (the host part of mesh.py:82 `apply_obb`), so the host hulls of run
 * k+1 overlap the device work of run k.  Prepared hulls are used only if the batch is unchanged
 * (any sh_upload_meshes / sh_synth_batch / sh_store("verts") voids them); sh_discard_prepared
 * drops them explicitly (the next run then does its host phase inline).  Results are identical
 * either way.  Off by default. */
/* Where the convex hull of SH_STAGE_OBB (`Trimesh.apply_obb()` -> qhull, mesh.py:82) is computed: "host" (quickhull on a
 * process-wide pool of worker threads, points read back through the device prefilter; hidden behind the previous run with
 * sh_set_overlap), "device" (round-based quickhull, k_hull.h: nothing leaves the GPU; a humerus it gives up -- more than 8 192
 * prefilter survivors, a horizon pinched by nearly coplanar points -- is re-done ALONE from inside sh_run / sh_collect: host
 * quickhull for that humerus, its stages re-run as a window of one behind whatever else is in flight; it stays on the host
 * hull while the batch is resident) or "auto" (default, also SHOULDER_HULL: host while the rank has enough usable hardware
 * threads -- 16 for a single rank, 48 per rank with LOCAL_WORLD_SIZE > 1; affinity mask and cgroup CPU quota counted).  Both give the
 * same triangles and the same record bits, hence bit-identical frames.  sh_get_hull_mode: 0 host, 1 device. */
int  sh_set_hull_mode(sh_ctx*, const char* mode);
int  sh_get_hull_mode(const sh_ctx*);
/* What "auto" resolves to for a context created by THIS process now (0 host, 1 device): usable hardware threads (affinity mask, cgroup
 * CPU quota) divided by LOCAL_WORLD_SIZE against 16 (a rank alone on its host) / 48 (several ranks).  Needs no device: a launcher can
 * size its lanes before it creates a context (bench.py: three lanes with the device hull, two with the host hull). */
int  sh_auto_hull_mode(void);
int  sh_set_overlap(sh_ctx*, int on);
int  sh_discard_prepared(sh_ctx*);

/* Several contexts on ONE device ("lanes": own stream, own scratch; consecutive batches go to alternating contexts
 * through sh_submit / sh_collect).  Their streams overlap on the device: the launch- and latency-bound geometry
 * kernels of one run execute beside the chip-filling UNet kernels of another (measured at B = 64: 14.2 -> 11.5 ms per
 * batch with two contexts).  Two UNet passes side by side gain nothing, each just takes twice as long; contexts that
 * turn this on chain their UNet passes with events in the order the host enqueued them, so a UNet pass only ever
 * shares the device with geometry.  Results are identical either way.  Off by default.
 * The HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams on
 * one queue run in order: a process that also runs torch / RCCL streams should export GPU_MAX_HW_QUEUES=16 before HIP
 * initialises (bench.py does). */
int  sh_set_unet_turns(sh_ctx*, int on);

#ifdef __cplusplus
}
#endif
#endif /* SHOULDER_HIP_H */
