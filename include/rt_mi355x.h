/*
 * rt_mi355x.h -- C ABI of the MI355X-native render hot path (libray_mi355x.so).
 *
 * This is the "internal" surface the Futhark-shaped drop-in boundary (include/ray.h)
 * is built on.  It mirrors the reference's language-level call surface
 *
 *     render(objs, width, height, cam) -> [pixel]
 *       futhark/ray.fut:166-169 (render_image), :241-247 (prepare_scene / render)
 *       rust/src/lib.rs:430-444, haskell/Raytracing.hs:187-190
 *
 * with plain pointers and sizes only (no torch / HIP types in any signature; a HIP
 * stream is passed as an opaque void*).  Every entry returns 0 on success and a
 * non-zero code on failure; rt_last_error() gives the message (the reference's
 * harness convention: `assert(ret == 0)`, futhark/main.c:74,97,116,131).
 *
 * All rendering entries ENQUEUE work on the context's stream and return; the
 * completion point is rt_context_sync() (futhark_context_sync, main.c:98,117).
 * There is no CPU fallback: without a usable HIP device context creation fails.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_context rt_context;    /* one device + one stream + work-queue state */
typedef struct rt_scene rt_scene;        /* `scene` (ray.fut:171-174): spheres + look_from/look_at/fov, host */
typedef struct rt_prepared rt_prepared;  /* `prepared_scene` (ray.fut:239): device-resident BVH + camera */

/* Kernel families (rt_context_set_variant).  All produce bit-identical pixels. */
enum {
  RT_VARIANT_AUTO = 0,        /* the pooled family; the pixel family for scenes beyond its limits: 2^22 spheres or more
                                 (a pooled work item is one dword, (node or leaf << 8) | ray slot) or a tree deeper than
                                 64 levels (the per-wave box stack no longer fits LDS) -- ~2 Gray/s instead of 6-16 */
  RT_VARIANT_PIXEL = 1,       /* one thread per pixel, BVH in HBM/L2, no LDS staging (BASELINE configs[1]) */
  RT_VARIANT_PERSISTENT = 2,  /* CROSS-CHECK family, selected by nothing: one ray per lane, work queue + in-place lane
                                 refill + phase voting.  A structurally different implementation of the same fold that
                                 the parity suite renders every case through; 5-15x slower than the pooled family */
  RT_VARIANT_POOLED = 3       /* persistent waves whose lanes share LDS work lists of (ray slot, node) items: any lane
                                 tests any ray's node; ballot/mbcnt compaction; work queue of tiles, or of the view's
                                 pixels sorted by bounce-chain length (BASELINE configs[2..4]) */
};

/* ---- context ------------------------------------------------------------------ */
/* device < 0: the current HIP device.  use_caller_stream == 0: the context creates and
 * owns a non-blocking stream (hip_stream is ignored).  use_caller_stream != 0: all work is
 * enqueued on the caller's hipStream_t `hip_stream` -- NULL then means the default stream
 * (which is what torch.cuda.current_stream().cuda_stream is unless the caller switched). */
int rt_context_create(rt_context **out, int device, void *hip_stream, int use_caller_stream);
int rt_device_count(void);   /* usable HIP devices (0: none -- there is no CPU path) */
/* One process, several devices: `devices[0..ndev)` are HIP device ordinals.  The context
 * behaves like a single-device one on devices[0] -- scenes, prepare_scene, render, sync, values -- but
 * prepare_scene replicates the scene on every device and rt_render / rt_render_image cut the frame into
 * cyclic tiles of 8 rows (part i of ndev on devices[i]) and gather the parts on devices[0]: RCCL
 * point-to-point over xGMI (librccl is loaded on demand), peer copies, or -- option "gather" = 3 -- no gather at
 * all: every device stores its pixels straight into the image on devices[0] over xGMI while it renders (peer
 * access; rt_render_part_inplace).  Option "gather": 0 auto (direct stores when every device can reach devices[0],
 * else RCCL, else peer copies), 1 peer copies, 2 RCCL, 3 direct stores.  A device may be listed more than once
 * (no RCCL then): that is how the fan-out is tested on a one-GPU box.  rt_render_part with nparts > 1 is refused
 * on such a context. */
int rt_context_create_multi(rt_context **out, const int *devices, int ndev);
int rt_context_num_devices(const rt_context *ctx);          /* 1 for an ordinary context */
const char *rt_context_gather_mode(rt_context *ctx);        /* "none", "direct-store", "rccl" or "peer-copy" (static strings) */
int rt_context_rccl_ranks(rt_context *ctx);                 /* ranks of the RCCL communicator behind the gather (0: RCCL is not what carries it) */
void rt_context_destroy(rt_context *ctx);
const char *rt_last_error(const rt_context *ctx);       /* "" when no error; owned by ctx */
/* What the last render entry of this context enqueued, for benches and profiles that want to assert which kernel ran (pixels never
 * depend on it).  Owned by ctx; "" before the first render.  (A multi-device context: the first device's part.)  Values:
 *   "family=none (memset)"        max_depth == 0: every pixel is the initial colour, no kernel
 *   "family=none (no rays)"       a caller-ray entry with n == 0
 *   "family=pixel (rays)" | "family=intersect" | "family=occluded" | "family=camera-rays"   the caller-ray entries (below)
 *   "family=intersect (per-ray)" | "family=occluded (per-ray)"   their lane kernels with per-ray intervals (rt_*_rays_ranged)
 *   "family=multi-hit k=K" | "family=multi-hit k=K (per-ray)"   rt_multi_hit_rays / rt_multi_hit_rays_ranged (K: the caller's k)
 *   "family=sweep k=K" [" (per-query)"] [" exclude"]   rt_sweep_spheres / rt_sweep_spheres_ranged (K: the caller's k)
 *   "family=nearest k=K[ pruned][ (per-point)]" | "family=none (no points)"   rt_nearest_spheres / rt_nearest_spheres_ranged (below)
 *   "family=within count|fill[ (per-point)][ first][ self]"   rt_spheres_within_count / _fill, rt_contact_pairs_count / _fill (" self"; below)
 *   "family=clusters"             rt_contact_clusters (below)
 *   "family=boxes count|fill[ (per-box)][ first]"   rt_spheres_in_boxes_count / _fill (below)
 *   "family=planes count|fill k=K[ (per-query)][ first]"   rt_spheres_in_planes_count / _fill (below; K: the caller's nplanes)
 *   "family=along count|fill[ (per-query)][ exclude][ first]"   rt_spheres_along_rays_count / _fill (below)
 *   "<the unmasked entry's string> masked[ mask=per-query]"   rt_intersect_rays_masked, rt_occluded_rays_masked, rt_nearest_spheres_masked,
 *         rt_spheres_within_masked_count / _fill (below): "family=intersect|occluded[ (per-ray)]", "family=nearest k=K[ pruned][ (per-point)]" or
 *         "family=within count|fill[ (per-point)][ first]", then " masked", then " mask=per-query" with mask_dev -- e.g.
 *         "family=within fill (per-point) first masked mask=per-query".  The masked occlusion entry always runs its lane kernel.
 *   "family=pairs targets|directions[ mask][ count][ words/wave=K]"   rt_visible_pairs / rt_visible_pairs_shaped (below; K: the caller's words_per_wave)
 *   "family=none (no rows)"       the part owns no row of the image
 *   "family=pixel" | "family=pixel (instrumented)" | "family=persistent"
 *   "family=pooled tickets=T instantiation=I[+CULL] frames=.. tiles=.. grid=.. waves=.. counters=..[(turns)] deep_class=.. deep_split=.. recording=0|1|2[ nodes=sign-ordered|planes,entry=lists|root,dark=0|1,leaf_box=0|1]"
 *     T = rays (rt_trace_rays: blocks of 64 caller rays, instantiation plain[+SPILL]; rt_occluded_rays: instantiation any[+SPILL]; rt_occluded_rays_ranged:
 *         the same, with " intervals=per-ray" appended to the string) | pixel-list | tiles-ordered | tiles-bit-reversed (a view's first frame with nothing to borrow, first_order = 1) | tiles-raster,
 *         followed by "(borrowed)" when the order / list is another view's (a new view of a prepared scene that has rendered a view of the same shape)
 *     I = plain | SOLO | COLD | COLD+SOLO | DONATE | DONATE+SOLO | ORD | ORD+SOLO | ORD+DONATE | ORD+SOLO+DONATE;  +CULL: boxes tested against the best hit so far; +SPILL: a box stack that may overflow into device memory (twenty waves per CU, trees taller than 15 levels)
 *     recording: 0 nothing, 1 the tiles' longest chains, 2 also every pixel's chain length
 *     nodes (render launches): the layout of the node records staged in LDS -- sign-ordered: the plain instantiations on a scene that is in LDS whole; planes: every other launch
 *     entry (render launches, in the same token: "nodes=sign-ordered,entry=lists"): lists = a new primary ray starts at its 8 x 8 tile's entry list -- at most one inner node and
 *         six leaves that the root walk of every ray of the tile provably reaches -- instead of at the root (option entry_lists: -1, the default, launches of the
 *         instantiation that exists with such lists -- plain tile tickets, 16 waves, the scene in LDS whole -- whose tiles are 8 consecutive image rows, while options
 *         leaf_box and dark_stop are both on: the kernel with lists has the leaf filter and the dark stop compiled in, so leaf_box = 0 or dark_stop = 0 turns the lists
 *         off, too -- a launch that says dark=0 or leaf_box=0 for a reason of its own, a recording launch or a camera outside the filter's guard, keeps its lists through
 *         a twin of the kernel that reads the two flags; 0 never; 1 every launch of that instantiation, with a flag at 0 through that twin); root = every ray starts at the root
 *     dark (render launches, in the same token: "nodes=planes,entry=root,dark=1"): 1 = the launch finishes a bounce chain whose light is exactly (0, 0, 0) as pixel 0 instead of tracing it on --
 *         the pixel it ends in whatever it meets (option dark_stop: -1, the default, every render launch that does not record; 0 never; 1 also rt_render_trace's instrumented launch);
 *         0 = full chains: every recording launch (recording != 0), dark_stop = 0
 *     leaf_box (render launches, in the same token: "nodes=planes,entry=root,dark=1,leaf_box=1"): 1 = BOX / BOX2 append a leaf child only if the sphere's own box, widened by a proven
 *         margin and kept in the leaf child's slot of the node record, passes (option leaf_box: -1, the default, every render launch whose scene and cameras pass the guards of
 *         DESIGN.md 3.4a and whose instantiation was compiled with the filter; 0 never; 1 also rt_render_trace's instrumented launch); 0 = every leaf child of a passing node is tested */
const char *rt_context_last_launch(const rt_context *ctx);
/* Under option "entry_count" = 1 a launch that says entry=lists runs a counting twin of its kernel (same pixels): per wave, the primary rays that started from their
 * tile's list and those that had a list but took the root because the lists of the rays their wave started together would not fit its leaf list.  The counts of the
 * context's LAST pooled render launch, summed, and per wave {lists, fallbacks} into per_wave[2 * cap_waves] when given; *waves = 0: that launch counted nothing
 * (no table, or the option off).  Synchronises the context. */
int rt_context_entry_counts(rt_context *ctx, uint64_t *lists, uint64_t *fallbacks, int64_t *waves, uint64_t *per_wave, int64_t cap_waves);
/* What rt_context_last_launch's line has no field for.  Of the context's LAST pooled render launch: *colour_lds = 1 when its kernel staged the colour table in LDS
 * and read the winner's colour there (an entry=lists launch with both flags set whose table fits next to 16 waves; option "col_lds" = 0: never), *flags_const = 1
 * when its kernel had the leaf filter and the dark stop compiled in (below); both 0 for entry=root.  Of the context: *tables_built = tables of entry lists its
 * launches have built, *tables_kept = launches that found their view's table in place -- a view (size, partition, bounce limit, camera) keeps the table its first
 * entry=lists launch built until the scene is updated, the leaf filter it was built under changes or the view is evicted; a batch with a camera per frame has no
 * view and builds its table per launch (option "entry_keep" = 0: every launch does).  Any pointer may be NULL.  No device work. */
int rt_context_entry_info(rt_context *ctx, int32_t *colour_lds, int32_t *flags_const, uint64_t *tables_built, uint64_t *tables_kept);
/* Exit lists (option "exit_lists": -1, the default, and 1: every launch of the kernel that has the leaf filter and the dark stop compiled in and the colours in
 * LDS, where the tables fit next to its 16 waves; 0: never): a ray that has just scattered starts at the list of the sphere it leaves -- a node of even depth
 * <= *dmax on that sphere's chain, and the siblings of the chain above it two to a record -- when it passes that node's box, else at the root (same
 * pixels, fewer box tests).  Of the context's LAST pooled render launch: *active = 1 when its scattered rays did; under option "entry_count" = 1 also *lists = the
 * scattered rays that started from a list and *fallbacks = those that had one and took the root (both 0 otherwise).  Of the context: *tables_built = times its
 * launches built the tables, *tables_kept = launches that found their scene's tables in place (a context keeps the tables of the last tree it rendered;
 * rt_prepared_update_spheres makes a new tree).  *dmax is a compile-time constant.  Any pointer may be NULL.  Synchronises the context when it reads counts. */
int rt_context_exit_info(rt_context *ctx, int32_t *active, int32_t *dmax, uint64_t *tables_built, uint64_t *tables_kept, uint64_t *lists, uint64_t *fallbacks);
/* The twenty-wave shape (option "wide_waves": workgroups of four waves, five per CU, no scene prefix in LDS, two ray planes): its plain, CULL and spilling
 * kernels exist a second time with those constants compiled in (same pixels).  Option "wide_const": -1, the default: every render launch of that
 * shape runs the twin; 0: the generic four-wave kernels.  rt_context_last_launch reads the same either way; *shape_const = 1 when the context's LAST pooled launch
 * ran a twin.  The pointer may be NULL.  No device work. */
int rt_context_wide_info(rt_context *ctx, int32_t *shape_const);
int rt_context_sync(rt_context *ctx);
/* Threads: every entry that takes a context holds that context's lock for the duration of the call (as a Futhark context does:
 * SURVEY.md 8b) -- host threads may share a context, a prepared scene and a scene; their calls are serialised and their frames
 * run on the context's one stream in the order the calls were admitted.  rt_last_error / rt_context_last_launch return
 * pointers into the context: read them before another thread's call replaces the string (or use a context per thread). */
int rt_context_set_variant(rt_context *ctx, int variant);
/* Tuning knobs by name (see DESIGN.md "knobs"); unknown name -> error.  None changes a pixel.  Among them "dark_stop" (-1 | 0 | 1, see rt_context_last_launch above):
 * rt_render_stats always counts the reference's full chains; rt_render_trace counts the stopped chains under dark_stop = 1 only.  "leaf_box" (-1 | 0 | 1) likewise:
 * rt_render_trace's leaf items are the reference's sphere tests unless leaf_box = 1.  "entry_lists" (-1 | 0 | 1): see rt_context_last_launch above; the instrumented launches
 * always start at the root.  "exit_lists" (-1 | 0 | 1): see rt_context_exit_info above.  "entry_keep" (-1 | 0) and "col_lds" (-1 | 0): see rt_context_entry_info above -- 0 builds the table of entry lists in every launch / loads the
 * winner's colour from memory in every launch. */
int rt_context_set_option(rt_context *ctx, const char *name, int64_t value);
int rt_context_device_info(const rt_context *ctx, int *device, int *num_cu, int *lds_bytes, char *name, int name_len);

/* ---- scenes (ray.fut:176-237) -------------------------------------------------- */
int rt_scene_rgbbox(rt_context *ctx, rt_scene **out);
int rt_scene_irreg(rt_context *ctx, rt_scene **out);
/* The irreg generator with its constants exposed: n x n spheres, extent k, y = 0.
 * irreg == (100, 600); SURVEY 8(d) "big" == (1000, 6000). */
int rt_scene_floor(rt_context *ctx, rt_scene **out, int n, float k);
/* Arbitrary scene: spheres7 = n x {pos.xyz, colour.xyz, radius}. */
int rt_scene_from_spheres(rt_context *ctx, rt_scene **out, const float *spheres7, int64_t n,
                          const float look_from[3], const float look_at[3], float fov);
int64_t rt_scene_num_spheres(const rt_scene *scene);
int rt_scene_free(rt_context *ctx, rt_scene *scene);

/* ---- prepare_scene (ray.fut:241-244): BVH build + camera, on the device ------------------
 * Values are tied to their context, as in the Futhark C API: the first prepare_scene of a scene
 * uploads its spheres to the context's device (the scene is device resident from then on), the
 * prepared scene's arrays live in the context's memory pool -- free it with the SAME context,
 * before that context is destroyed. */
int rt_prepare_scene(rt_context *ctx, rt_prepared **out, int64_t h, int64_t w, const rt_scene *scene);
int rt_prepared_free(rt_context *ctx, rt_prepared *ps);
int64_t rt_prepared_num_spheres(const rt_prepared *ps);
int32_t rt_prepared_height(const rt_prepared *ps);   /* levels of inner nodes on the longest root-to-leaf path */
/* Canonical `bvh = {L, I}` (bvh.fut:28) copied back from the device for parity checks.
 * L7: n x 7 floats; bmin/bmax: (n-1) x 3; left/right: (n-1) encoded ptr (inner i -> i,
 * leaf i -> -2 - i); parent: (n-1).  Any pointer may be NULL. */
int rt_prepared_get_bvh(rt_context *ctx, const rt_prepared *ps, float *L7, float *bmin, float *bmax,
                        int32_t *left, int32_t *right, int32_t *parent);
int rt_prepared_get_camera(rt_context *ctx, const rt_prepared *ps, float cam12[12]);

/* ---- scenes from spheres in device memory: prepare, and update in place ---------------------------------------------
 * spheres7_dev: n x 7 float32 {pos.xyz, colour.rgb, radius} in the context's device memory (a hipMalloc'd buffer, a torch tensor).
 * A scene prepared from device spheres, or updated to them, is indistinguishable from rt_scene_from_spheres + rt_prepare_scene on
 * the same bytes: the BVH arrays (rt_prepared_get_bvh, byte for byte), the tree height, the camera, the culling guards and with them
 * every later launch's instantiation (rt_context_last_launch), every pixel and every caller-ray output, under every variant.  Spheres
 * with NaN / inf components or a radius below 2^-20 are accepted as that route accepts them (the same BVH bytes; culling off).
 * Both entries run on the context's stream and return after the build has completed: the caller may then overwrite or free
 * spheres7_dev -- nothing of the prepared scene points at it.  The option gpu_build = 0 copies the spheres to the host and builds there.
 * Refused (non-zero, rt_last_error set, nothing launched, ps unchanged): a NULL pointer, h or w <= 0, n < 2 or n > 2^26 (as
 * rt_scene_from_spheres), a multi-device context. */
int rt_prepare_scene_device(rt_context *ctx, rt_prepared **out, int64_t h, int64_t w, const float *spheres7_dev, int64_t n,
                            const float look_from[3], const float look_at[3], float fov);
/* The BVH of ps rebuilt in place from n new spheres (same n, same camera, same handle and device block).  It first drains the work
 * on the context's streams that may still read the old arrays, then puts every view of ps (tile orders, pixel lists, class tables)
 * back into the state of a view never rendered.  Refused as above, and also: n != rt_prepared_num_spheres(ps), and ctx other than the
 * context that prepared ps.  The caller must not render ps through another context while an update is in flight, and must have
 * synchronised any other context that rendered it.  After a HIP failure (not a refusal) the scene's contents are unspecified: free it. */
int rt_prepared_update_spheres(rt_context *ctx, rt_prepared *ps, const float *spheres7_dev, int64_t n);

/* ---- render (ray.fut:246-247 -> render_image :166-169) -------------------------- */
/* Whole image: out_dev = device pointer to h*w int32, row-major from the top row. */
int rt_render(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t *out_dev);
/* Row-tile partition for multi-GPU: the image is cut into tiles of rows_per_tile rows;
 * part p of nparts renders tiles t with t % nparts == p, packed in tile order into
 * out_dev (rt_part_rows(h, rows_per_tile, p, nparts) * w int32).  max_depth: the
 * reference's bounce limit is 50 (ray.fut:154). */
int rt_render_part(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth,
                   int32_t rows_per_tile, int32_t part, int32_t nparts, int32_t *out_dev);
/* The language-level surface itself: render_image objs width height cam (ray.fut:166) with an
 * explicit camera (12 floats: origin, llc, horizontal, vertical; ray.fut:88-91) instead of the
 * one prepare_scene derived.  cam12 == NULL: the prepared camera, at any h x w -- as `render h w
 * prepared` does in the reference (ray.fut:246): the aspect ratio stays the one prepare_scene was given. */
int rt_render_image(rt_context *ctx, const rt_prepared *objs, int64_t width, int64_t height, const float cam12[12],
                    int32_t max_depth, int32_t rows_per_tile, int32_t part, int32_t nparts, int32_t *out_dev);
/* Throughput entry: `nframes` frames of one prepared scene in ONE launch (a camera path, or the same view again and
 * again as the reference's harness does, main.c:107-124).  Frame f is traced through cams12 + 12 f (host memory; NULL:
 * the prepared camera for every frame) into out_dev + f * frame_stride (int32 elements, >= rows * w).  The persistent
 * waves run straight across frame boundaries, so a launch's fill and drain are paid once per batch instead of once
 * per frame.  Partition arguments as rt_render_part.  The array at cams12 is copied before the call returns.
 * Limits (refused, nothing launched): 1 <= nframes <= 4096; nframes * frame_stride < 2^31; and tiles per frame x nframes < 2^26, where
 * a frame (a part: its rows) has ceil(rows / 8) x ceil(w / 8) tiles of 8 x 8 pixels -- the second limit implies the third for frames whose
 * sides are multiples of 8, but not for thin ones: 512 frames of 1 x 2^20 are refused by the third alone.  rt_render_part_inplace: the same.
 * On a multi-device context (part 0 of 1 only): every device renders its row tiles of ALL the frames in one launch, the
 * framebuffer gather moves nframes x part per device, one assembly launch writes the nframes images. */
int rt_render_batch(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth, int32_t rows_per_tile,
                    int32_t part, int32_t nparts, int32_t nframes, const float *cams12, int64_t frame_stride, int32_t *out_dev);
/* The same part of the same frames, but stored IN PLACE: image_dev is the FULL image (frame f at image_dev + f *
 * frame_stride, frame_stride >= h * w; 0 = h * w for one frame) and every pixel of the part goes to its place in it
 * -- no packed part buffer, no gather, no assembly launch.  image_dev may be memory of ANOTHER device of the node
 * (a peer allocation, or a buffer of another process mapped with rt_ipc_import): the 4-byte pixel stores then are
 * the framebuffer exchange of SURVEY.md 8(e) -- they cross xGMI while the frame is being traced instead of in a
 * gather behind it (futhark/main.c:107-135 has nothing to correspond: the reference is a single device).  The
 * caller orders the consumers of the image behind every part's stream (event, collective, barrier). */
int rt_render_part_inplace(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth, int32_t rows_per_tile,
                           int32_t part, int32_t nparts, int32_t nframes, const float *cams12, int64_t frame_stride,
                           int32_t *image_dev);
/* One process per GPU: the owner of an image exports the allocation (a pointer rt_device_alloc returned) as 64
 * opaque bytes (hipIpcMemHandle_t), the other processes import them and get a device pointer usable as image_dev
 * above; rt_ipc_close unmaps it (before the owner frees the buffer). */
int rt_ipc_export(rt_context *ctx, void *dev, unsigned char handle64[64]);
int rt_ipc_import(rt_context *ctx, const unsigned char handle64[64], void **out_dev);
int rt_ipc_close(rt_context *ctx, void *imported_dev);
int64_t rt_part_rows(int64_t h, int32_t rows_per_tile, int32_t part, int32_t nparts);
/* Scatter one part's packed rows into a full h*w image on the device (rank-0 side of
 * the framebuffer gather). */
int rt_place_part(rt_context *ctx, int64_t h, int64_t w, int32_t rows_per_tile, int32_t part, int32_t nparts,
                  const int32_t *part_dev, int32_t *image_dev);

/* The same for ALL parts at once: stacked_dev = nparts x pad_rows x w int32 (what a gather of the
 * ranks' padded send buffers delivers on rank 0), one kernel. */
int rt_place_parts(rt_context *ctx, int64_t h, int64_t w, int32_t rows_per_tile, int32_t nparts, int64_t pad_rows,
                   const int32_t *stacked_dev, int32_t *image_dev);
/* General form: part p's packed rows start at stacked_dev + p * part_stride (int32 elements), so one
 * gathered buffer may carry the parts of several frames (one gather per step, see dist.py). */
int rt_place_parts_strided(rt_context *ctx, int64_t h, int64_t w, int32_t rows_per_tile, int32_t nparts,
                           int64_t part_stride, const int32_t *stacked_dev, int32_t *image_dev);

/* ... and of a batch, in one launch: frame f's parts lie frame_stride_in elements behind frame f - 1's inside every
 * part (part_stride >= (nframes - 1) * frame_stride_in + the largest part), its image frame_stride_out (>= h * w)
 * elements behind the previous one at images_dev. */
int rt_place_parts_batch(rt_context *ctx, int64_t h, int64_t w, int32_t rows_per_tile, int32_t nparts, int64_t part_stride,
                         int32_t nframes, int64_t frame_stride_in, int64_t frame_stride_out, const int32_t *stacked_dev,
                         int32_t *images_dev);

/* Work counters of one frame, computed on the device by an instrumented launch of the
 * same traversal: rays (objs_hit calls), box tests, sphere tests. */
int rt_render_stats(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth,
                    uint64_t stats3[3]);

/* Diagnostic: one instrumented launch of the pooled kernel; per wave 16 x u64 = {wall clock (100 MHz ticks,
 * chip-wide) at start, at queue exhaustion, at exit; #BOX | #LEAF << 21 | #SHADE << 42 operations; shader
 * cycles lived; #BOXT | #BOX2 << 32 (both are counted in #BOX as well); (box items << 32 | leaf items); deepest bounce
 * chain finished | max box stack << 16 | max leaf list << 32; shader cycles spent inside BOX, BOX2, BOXT, LEAF, SHADE
 * operations (words 8..12); 13..15 reserved}. */
int rt_render_trace(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth,
                    uint64_t *records, int32_t max_waves, int32_t *num_waves);

/* Times `iters` back-to-back launches of rt_render_part with HIP events recorded on the
 * context's stream (after `warmup` untimed launches); ms_out[i] = duration of launch i. */
int rt_render_timed(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth,
                    int32_t rows_per_tile, int32_t part, int32_t nparts, int32_t *out_dev,
                    int32_t warmup, int32_t iters, float *ms_out);

/* ---- caller-supplied rays: objs_hit, occlusion and ray_colour (ray.fut:76-86, :126-148) on a prepared scene ------
 * Rays are n x 6 contiguous float32 in the context's device memory, {origin.xyz, dir.xyz}.  Every entry enqueues its
 * work on the context's stream and returns (completion: rt_context_sync), holding the context lock like the render
 * entries.  Refused (non-zero, rt_last_error set, nothing launched): n < 0, n >= 2^31, a NULL rays pointer, no output,
 * and a multi-device context.  n == 0 succeeds without a launch.  Results are the reference's, bit for bit, for every
 * ray with finite components and a non-zero direction; for other rays they are unspecified (but nothing is read or
 * written out of range). */
/* ray_colour objs r max_depth (ray.fut:126-148) of each ray, with objs_hit r 0 1e9 as the render path has it.
 * colour3_dev: n x 3 float32, the colour before colour_to_pixel; pixel_dev: n int32, colour_to_pixel of it
 * (ray.fut:156-162).  Either may be NULL, not both.  The pooled family traces the rays under RT_VARIANT_AUTO /
 * RT_VARIANT_POOLED (64 consecutive rays per ticket of its raster queue; the pixel family beyond its limits, as
 * rt_render); the pixel family, one lane per ray, under RT_VARIANT_PIXEL and RT_VARIANT_PERSISTENT.
 * rt_context_last_launch: "family=pooled tickets=rays ..." or "family=pixel (rays)". */
int rt_trace_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth,
                  float *colour3_dev, int32_t *pixel_dev);
/* objs_hit bvh r t_min t_max (ray.fut:76-86) of each ray: boxes tested with aabb_hit over (t_min, t_max), spheres folded
 * over (scene_epsilon, best) from best = t_max (ties to the lowest leaf index), the winner re-intersected over
 * (t_min, t + 1).  index_dev: n int32, the sphere's index in the prepared scene's L (rt_prepared_get_bvh), -1 for #none
 * (no sphere, or a failed re-intersection); hit7_dev: n x 7 float32 {t, p.xyz, normal.xyz} of the returned hit
 * (ray.fut:40-46), seven zeros for #none; may be NULL.  Refused as well: t_min or t_max non-finite or negative,
 * t_min > t_max, t_max > 1e9.  One lane per ray (rt_context_last_launch: "family=intersect"). */
int rt_intersect_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                      int32_t *index_dev, float *hit7_dev);
/* Occlusion (any-hit) of each ray over (t_min, t_max): occluded_dev[i] = 1 iff some leaf j of the prepared scene's BVH has
 * every inner node on its root path passing aabb_hit node r t_min t_max (ray.fut:53-70) and sphere_hit L[j] r t_min t_max
 * is #some (ray.fut:32-51: root1 or root2 strictly inside (t_min, t_max)); else 0.  n bytes.  This is bvh_fold
 * (bvh.fut:61-84) with that fixed interval and a logical OR of the sphere tests: it does not depend on the order of the
 * walk, so a ray stops at its first accepted sphere.  The caller's t_min bounds the spheres (objs_hit's fold uses
 * scene_epsilon instead); with t_min = 0.1 the result is rt_intersect_rays(.., 0.1, t_max) index >= 0 for every ray whose
 * closest accepted root is below 2^23.  A shadow ray from p to a point light L: d = L - p over (eps, 1).  Refused as
 * rt_intersect_rays is (interval included), and for a NULL occluded_dev; t_min == t_max gives all zeros.  The pooled
 * family's any-hit loop under RT_VARIANT_POOLED ("family=pooled tickets=rays instantiation=any..."), one lane per ray under
 * RT_VARIANT_PIXEL / RT_VARIANT_PERSISTENT ("family=occluded").  RT_VARIANT_AUTO: the pooled loop when the whole scene is
 * staged in LDS and t_max > 1, where it was measured faster; otherwise (and beyond the pooled family's limits) the lane kernel. */
int rt_occluded_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                     uint8_t *occluded_dev);
/* The same two queries with an interval per ray: t_min_dev and t_max_dev are n float32 each in the context's device memory, and
 * ray i gets exactly what rt_intersect_rays / rt_occluded_rays give it alone at (t_min_dev[i], t_max_dev[i]), bit for bit, under
 * every variant and launch shape.  The intervals are device data and are not read back: a ray whose interval fails
 * 0 <= t_min <= t_max <= 1e9 (NaN, +-inf and t_min > t_max included) is answered as a miss -- index -1 and seven zero floats,
 * occluded 0 -- and its walk does not start.  -0.0 behaves as 0.0.  Refused as the scalar entries are (n out of range, NULL rays
 * or output pointer, a multi-device context), and for a NULL t_min_dev or t_max_dev.
 * rt_intersect_rays_ranged: one lane per ray ("family=intersect (per-ray)").
 * rt_occluded_rays_ranged: the pooled family's any-hit loop in its per-ray mode under RT_VARIANT_POOLED ("family=pooled tickets=rays
 * instantiation=any[+SPILL] ... intervals=per-ray"), the lane kernel ("family=occluded (per-ray)") under RT_VARIANT_PIXEL /
 * RT_VARIANT_PERSISTENT.  RT_VARIANT_AUTO: the lane kernel (the host cannot see t_max; measured).
 * Raising t_min is NOT depth peeling: objs_hit folds the spheres over (scene_epsilon, best) whatever t_min is, so a sphere nearer
 * than t_min still wins the fold (and then fails its re-intersection: #none) -- it does not skip to the next sphere (rt_multi_hit_rays,
 * below, gives the surfaces behind the first). */
int rt_intersect_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *t_min_dev,
                             const float *t_max_dev, int32_t *index_dev, float *hit7_dev);
int rt_occluded_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *t_min_dev,
                            const float *t_max_dev, uint8_t *occluded_dev);
/* Multi-hit: the k nearest sphere crossings of each ray -- what lies behind the first hit (layers, entry and exit points, crossing
 * counts).  The crossings of ray r over (t_min, t_max) are every (t, j, root) with leaf j visited (every inner node on its root path
 * passes aabb_hit node r t_min t_max, the leaves rt_occluded_rays reaches) and t = root 1 (-b - sq)/a or root 2 (-b + sq)/a of
 * sphere_hit L[j] r (ray.fut:32-51) strictly inside (t_min, t_max); a sphere gives up to two, entry and exit.  They are ordered by t,
 * then j, then root, all ascending.  count_dev: n int32, the number of crossings (not capped at k; > 0 iff rt_occluded_rays gives 1).
 * The first min(count, k) crossings, row-major per ray: index_dev n x k int32 (j), root_dev n x k uint8 (1 or 2), hit7_dev n x k x 7
 * float32 {t, p.xyz, normal.xyz} (rt_intersect_rays's arithmetic: p = o + t d, normal = (1 / radius) (p - centre)); the slots past
 * min(count, k) are -1, 0 and seven zero floats.  Any output may be NULL, not all four.  Exact, bit for bit, for every k: the answer for
 * k = a is a prefix of the answer for k = b > a.  No culling and no early exit: every visited sphere is tested.  Refused (nothing
 * launched): as rt_intersect_rays (n out of range, NULL rays, a multi-device context, the scalar interval rule), and k < 1 or k > 32.
 * One lane per ray under every variant (rt_context_last_launch: "family=multi-hit k=<k>").
 * rt_multi_hit_rays_ranged: the interval of ray i is (t_min_dev[i], t_max_dev[i]), as rt_intersect_rays_ranged -- a ray whose interval
 * fails 0 <= t_min <= t_max <= 1e9 is a miss (count 0, every slot padded), -0.0 behaves as 0.0; refused also for a NULL t_min_dev or
 * t_max_dev ("family=multi-hit k=<k> (per-ray)").  Unlike raising t_min in rt_intersect_rays, this is depth peeling: crossing s + 1 is
 * the next surface behind crossing s. */
int rt_multi_hit_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                      int32_t k, int32_t *count_dev, int32_t *index_dev, uint8_t *root_dev, float *hit7_dev);
int rt_multi_hit_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev,
                             const float *t_min_dev, const float *t_max_dev, int32_t k,
                             int32_t *count_dev, int32_t *index_dev, uint8_t *root_dev, float *hit7_dev);
/* Sphere casts (sweeps): the first k contacts of a MOVING sphere -- continuous collision detection, a character or probe volume, a thick
 * ray.  A query is a ray {o, d} (the n x 6 float32 layout of the ray queries), a radius rq and an interval (t_min, t_max): o is the moving
 * sphere's centre at t = 0, d its displacement per unit t.  It meets sphere j of L (centre c, radius r) exactly where the ray of its
 * centre meets the sphere (c, r + rq), so, in binary32 without contraction:
 *     R = r + rq;  t1 = (-b - sq) / a, t2 = (-b + sq) / a: the two roots of sphere_hit (ray.fut:32-51) of the ray against (c, R), the
 *     arithmetic of rt_multi_hit_rays with R in place of the radius; a discriminant <= 0 gives no contact, NaN roots pass no compare below.
 *     Entry contact:         if t1 > t_min, the contact is tau = t1, start = 0, accepted iff t1 < t_max.
 *     Overlap at the start:  otherwise, if t2 > t_min and t_min < t_max, the contact is tau = t_min (-0.0 reported as +0.0), start = 1: the
 *                            moving sphere already overlaps j where the interval begins (the physics engines' convention: an initial
 *                            overlap is a hit at distance zero).
 *     Otherwise none (touching only at the exit, t2 == t_min, is none).  A sphere gives at most one contact.
 *     A STATIONARY query, d = (+-0, +-0, +-0), has no contact at all, not even with a sphere it rests inside: a = b = 0, so the discriminant
 *     is 0 - 0 * c = 0 (NaN where c overflows), which is not positive.  Ask rt_spheres_within_* at p = o with bound rq for those overlaps.
 * Sphere j is consulted iff every inner node on its root path passes aabb_hit (ray.fut:53-70) over (t_min, t_max) on the node's box WIDENED
 * by rq per component, fl(lo_k - rq) and fl(hi_k + rq).  With rq = 0 (or -0.0) these are exactly the leaves rt_multi_hit_rays visits.  Like
 * every ray query here this inherits the reference's partial boxes: on a tree taller than the AABB propagation's floor(log2 n) + 2 sweeps
 * the nodes nearest the root do not contain their subtrees, and a sphere under a box the widened test fails is not consulted.
 * The contacts of a query are ordered by (tau, j), ascending: several start overlaps come first, in ascending j (rt_spheres_within_* at
 * p = o + t_min d with bound rq enumerates them all).  count_dev: n int32, all contacts (not capped at k).  The first min(count, k),
 * row-major per query: index_dev n x k int32 (j), start_dev n x k uint8 (0 entry contact, 1 overlap at the start), hit7_dev n x k x 7
 * float32 {tau, p.xyz, normal.xyz}: p = o + tau d is the moving sphere's CENTRE at contact, normal = (1.0f / R) * (p - c), one division per
 * written slot (the touching point on the scene sphere is c + r * normal: left to the caller).  The slots past min(count, k) are -1, 0 and
 * seven zero floats.  Any output may be NULL, not all four.  Exact, bit for bit, for every k: the answer for k = a is a prefix of the answer
 * for k = b > a; k = 1 is the classic sphere cast.  The interval is never narrowed by the contacts found.
 * Refused (non-zero, rt_last_error set, nothing launched): as rt_multi_hit_rays (n out of range, NULL rays, a multi-device context, the
 * scalar interval rule, k < 1 or k > 32), and a radius that is not finite or outside [0, 1e9].  n == 0 succeeds without a launch.  One lane
 * per query under every variant (rt_context_last_launch: "family=sweep k=<k>").
 * rt_sweep_spheres_ranged: query i has its own radius_dev[i], t_min_dev[i], t_max_dev[i] (n float32 each; a NULL one is refused).  A query
 * whose interval fails 0 <= t_min <= t_max <= 1e9 or whose radius fails 0 <= radius <= 1e9 (NaN, +-inf included) is a miss: count 0, every
 * slot padded, its walk does not start; -0.0 behaves as 0.0.  exclude_dev: NULL, or n int32 -- sphere exclude_dev[i] is skipped at the leaf
 * (one compare: neither counted nor listed); a value outside [0, num_spheres) excludes nothing.  This lets a scene sweep its own spheres:
 * query i is the centre and radius of L[i], d its velocity times the time step, exclude = i.  rt_context_last_launch: "family=sweep k=<k>
 * (per-query)", then " exclude" when exclude_dev is given. */
int rt_sweep_spheres(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius, float t_min, float t_max,
                     int32_t k, int32_t *count_dev, int32_t *index_dev, uint8_t *start_dev, float *hit7_dev);
int rt_sweep_spheres_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *radius_dev,
                            const float *t_min_dev, const float *t_max_dev, const int32_t *exclude_dev, int32_t k,
                            int32_t *count_dev, int32_t *index_dev, uint8_t *start_dev, float *hit7_dev);
/* Ray paths: the mirror-bounce chain of each ray -- the sequence of spheres and hit points ray_colour (ray.fut:126-148) follows through up to
 * max_depth bounces, exactly as the render path and rt_trace_rays run it (binary32, no contraction, the reference's association order).
 * Iteration s = 0, 1, .. calls objs_hit objs r_s 0.0 1e9 (ray.fut:130, :76-86) on the current ray r_s, r_0 being the caller's; a #some hit is
 * VERTEX s: bit for bit what rt_intersect_rays(.., 0.0f, 1e9f, ..) returns for r_s -- the sphere's index in L and {t, p.xyz, normal.xyz} --
 * the (0.0, t + 1) re-intersection and ties to the lowest leaf included.  scatter (ray.fut:116-124): u = (1.0f / sqrtf(d.d)) * d,
 * refl = u - (2.0f * dot(u, normal)) * normal; the chain continues iff dot(refl, normal) > 0.0f, with r_{s+1} = {hit.p, refl} and
 * light = light * colour(L[j]) component-wise from (1, 1, 1).
 * count_dev: n int32, the number of vertices -- every objs_hit that returned #some, an absorbing last one included; never capped at k,
 *   0 <= count <= max_depth.
 * end_dev: n uint8, how the loop left.  RT_PATH_ESCAPED: the last objs_hit was #none.  RT_PATH_ABSORBED: the last vertex's scatter was #none.
 *   RT_PATH_TRUNCATED: max_depth vertices, each of which scattered (max_depth == 0: count 0, TRUNCATED).  The number of objs_hit calls is
 *   count + (end == RT_PATH_ESCAPED).
 * light3_dev (n x 3), last_ray6_dev (n x 6), colour3_dev (n x 3) float32: the loop variables light, r and the result at exit.  ESCAPED: r is the
 *   ray that missed, colour = light * sky(r).  ABSORBED: r is the ray that hit the absorbing vertex, light does not include that vertex's colour,
 *   colour = light * 0.  TRUNCATED: r is the scattered ray ray_colour never traced, light INCLUDES the last vertex's colour; colour is
 *   ray_colour's light * 0 with the light before that vertex.  colour3 is rt_trace_rays's colour3, bit for bit.
 * index_dev n x k int32, hit7_dev n x k x 7 float32, row-major per ray (64-bit offsets): the first min(count, k) vertices; the slots past
 *   them are -1 and seven zero floats.  The answer for k = a is a prefix of the answer for k = b > a.
 * Any output may be NULL, not all seven.  Refused (non-zero, rt_last_error set, nothing launched): as the other caller-ray entries (n out
 * of range, NULL rays, a multi-device context), k < 1 or k > 1024, max_depth < 0, and a rays_per_wave that is neither 0 nor a multiple of
 * 64 in [64, 4096].  n == 0 succeeds without a launch.  For a ray with a non-finite component or a zero direction the outputs are
 * unspecified, but its lane terminates, count <= max_depth, end is one of the three codes, nothing is read or written out of range and no
 * other ray's answer changes.
 * One lane kernel under every variant: a wave owns rays_per_wave consecutive rays and its lanes pick up the block's next ray when theirs
 * ends (chain lengths diverge: most rays end within four vertices, a few run to max_depth).  The shape changes no bit of the answer.
 * rt_trace_paths chooses it: 64 while n <= 64 * 8 * CUs, above that the smallest multiple of 64 that keeps the grid at 8 * CUs waves, at
 * most 256 (fitted to measurements: DESIGN.md 3.5h); rt_trace_paths_shaped takes it from the caller (0: the same rule).
 * rt_context_last_launch: "family=paths k=<k> depth=<max_depth> rays/wave=<R>". */
enum { RT_PATH_ESCAPED = 0, RT_PATH_ABSORBED = 1, RT_PATH_TRUNCATED = 2 };
int rt_trace_paths(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth, int32_t k,
                   int32_t *count_dev, uint8_t *end_dev, int32_t *index_dev, float *hit7_dev,
                   float *light3_dev, float *last_ray6_dev, float *colour3_dev);
int rt_trace_paths_shaped(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth, int32_t k,
                          int32_t *count_dev, uint8_t *end_dev, int32_t *index_dev, float *hit7_dev,
                          float *light3_dev, float *last_ray6_dev, float *colour3_dev, int32_t rays_per_wave);
/* ---- proximity: the spheres nearest to caller-supplied points ------------------------------------------------------------------
 * For a point p and sphere j of the prepared scene's L (centre c, radius r) the gap is the signed distance from p to the sphere's surface,
 * negative inside, as exactly this float32 arithmetic (no contraction, correctly rounded sqrtf):
 *     dx = p.x - c.x; dy = p.y - c.y; dz = p.z - c.z;   gap = sqrtf((dx*dx + dy*dy) + dz*dz) - r
 * Sphere j is selected for p iff gap <= max_dist; the selected spheres are ordered by (gap, j), both ascending.  This is brute force over ALL
 * spheres: it depends on no tree, builder or variant (the BVH walk only prunes boxes proven to hold no selected sphere).
 * points3_dev: n x 3 float32 in the context's device memory.  count_dev: n int32, the number of selected spheres (not capped at k).
 * index_dev: n x k int32, the first min(count, k) selected j, then -1; gap_dev: n x k float32, their gaps, then 0.0f (64-bit offsets).
 * Any output may be NULL, not all three.  The answer for k = a is a prefix of the answer for k = b > a.  count_dev == NULL is the k-nearest
 * mode: the walk also prunes by the k-th gap found so far; its slots are bit-identical to the same call's with count_dev set.  A point with a
 * non-finite component gets count 0 and every slot padded.  Exact, bit for bit, for scenes whose spheres are all finite with radius >= 0
 * (radius 0: plain k-nearest-neighbour search of the centres); for other scenes the result is unspecified, but nothing is read or written out
 * of range.  j is an index into L (Morton order): rt_prepared_get_sphere_ids maps it back to the caller's order.
 * Contacts: the spheres a query sphere (c_q, r_q) overlaps or touches are those selected for p = c_q, max_dist = r_q (gap <= r_q); the
 * self-contacts of a scene pass its own centres and radii (rt_nearest_spheres_ranged), and every sphere then finds itself at gap -r.
 * Refused (non-zero, rt_last_error set, nothing launched): n < 0 or n >= 2^31, NULL points3_dev, all outputs NULL, k < 1 or k > 32, a
 * multi-device context, max_dist outside [0, 1e9] or not finite (rt_nearest_spheres), NULL max_dist_dev (rt_nearest_spheres_ranged).  n == 0
 * succeeds without a launch ("family=none (no points)").  Enqueued on the context's stream (completion: rt_context_sync).  One lane per point
 * under every variant: rt_context_last_launch "family=nearest k=<k>", with " pruned" appended in k-nearest mode and " (per-point)" for
 * rt_nearest_spheres_ranged, whose point i has its own bound max_dist_dev[i] (n float32): an invalid one (NaN, +-inf, negative, above 1e9)
 * makes point i a miss; -0.0 behaves as 0.0. */
int rt_nearest_spheres(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                       int32_t k, int32_t *count_dev, int32_t *index_dev, float *gap_dev);
int rt_nearest_spheres_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev,
                              const float *max_dist_dev, int32_t k, int32_t *count_dev, int32_t *index_dev, float *gap_dev);
/* ---- range queries: EVERY sphere within a distance of caller-supplied points, and a scene's contact pairs, with no cap -----------------
 * The selection rule is rt_nearest_spheres's: sphere j of L is selected for point i iff gap <= the point's bound, gap being exactly the
 * float32 arithmetic above -- and, where first_dev is given, j >= first_dev[i].  Brute force over all spheres defines the answer; it is exact,
 * bit for bit.  A row has no length limit, so the answer comes in CSR form and in two phases, because its size is not known in advance:
 *   offsets : n + 1 int64.  offsets[0] = 0, offsets[i + 1] - offsets[i] = the number of spheres selected for point i, offsets[n] = the total.
 *             Without first_dev a row's length is rt_nearest_spheres's count_dev[i] for the same point and bound.
 *   index   : total int32.  Row i at [offsets[i], offsets[i + 1]): the selected j in ASCENDING j -- not in (gap, j) order: the walk meets the
 *             leaves of the tree in ascending j, and a row of any length cannot be sorted in registers.  Sort rows yourself if you need
 *             them by gap.
 *   gap     : total float32, the gap of each entry.         point : total int32, the row number i of each entry (the COO form: (point,
 *             index) is the list of pairs).  Any of the three may be NULL, not all.
 * rt_spheres_within_count enqueues the count pass and the scan that writes offsets_dev[0 .. n] on the context's stream and returns without
 * synchronising.  The caller reads offsets_dev[n] (rt_copy_to_host), allocates that many entries and calls rt_spheres_within_fill with the
 * SAME points, bounds, first_dev and scene, and capacity = the entries it allocated.  _fill recomputes the selection and writes entry
 * offsets[i] + (rank of j in row i) only while it is below offsets[i + 1] and below capacity: offsets that belong to another query (or a
 * scene updated between the two calls) give an unspecified result, but never a write outside [0, capacity).
 * max_dist_dev == NULL: the scalar max_dist for every point; otherwise n float32, one bound per point, and the scalar is ignored.
 * first_dev == NULL: no lower index bound; otherwise n int32: first_dev[i] <= 0 selects from 0, first_dev[i] >= the sphere count gives an empty
 * row (the filter is a compare at the leaf; it prunes no subtree).  A point with a non-finite component, or a per-point bound that is NaN,
 * +-inf, negative or above 1e9, has an empty row; -0.0 behaves as 0.0.  Exact for scenes whose spheres are finite with radius >= 0; for other
 * scenes unspecified, but nothing is read or written out of range.
 * Contact pairs are the scene's self-query: point i is the centre of L[i], its bound fl(radius_i + margin), first = i + 1.  Pair (i, j), i < j,
 * is reported iff gap(centre_i, L[j]) <= fl(radius_i + margin) -- once, without (i, i).  The predicate is evaluated from the LOWER index only:
 * in float32 it need not be symmetric in the last bit, and (j, i) is never consulted.  offsets: n + 1 int64 for the scene's n spheres;
 * pair_dev: total x 2 int32, rows {i, j} in ascending (i, j); gap_dev: total float32, that gap (centre i to the surface of j; subtract radius_i
 * for the surface-to-surface distance); either may be NULL, not both.  A sphere whose bound is not in [0, 1e9] or whose centre is not finite
 * reports no pair as i.  i and j are indices into L: rt_prepared_get_sphere_ids maps them to the caller's order.
 * Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device context, n < 0 or n >= 2^31, NULL
 * points3_dev, NULL offsets_dev, a negative capacity, every output NULL, a scalar max_dist (when it is used) or a margin outside [0, 1e9] or
 * not finite.  n == 0 succeeds and _count still writes offsets_dev[0] = 0.  One lane per point under every variant; rt_context_last_launch:
 * "family=within count" / "family=within fill", then " (per-point)" with max_dist_dev, " first" with first_dev, " self" for the contact pairs. */
int rt_spheres_within_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                            const float *max_dist_dev, const int32_t *first_dev, int64_t *offsets_dev);
int rt_spheres_within_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                           const float *max_dist_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                           int32_t *index_dev, float *gap_dev, int32_t *point_dev);
int rt_contact_pairs_count(rt_context *ctx, const rt_prepared *ps, float margin, int64_t *offsets_dev);
int rt_contact_pairs_fill(rt_context *ctx, const rt_prepared *ps, float margin, const int64_t *offsets_dev, int64_t capacity,
                          int32_t *pair_dev, float *gap_dev);
/* ---- contact clusters: the connected components of the contact pairs' graph, reduced on the device ------------------------------------
 * The vertices are the scene's n spheres L[0 .. n) in Morton order; the edges are EXACTLY the rows rt_contact_pairs_fill reports at the same
 * margin (the one-sided float32 predicate above, evaluated from the lower index; a sphere whose bound is not in [0, 1e9] or whose centre is
 * not finite offers no edge as i, and may still be some lower sphere's j).  No pair is materialised: the walk of rt_contact_pairs_count unites
 * i and j in a lock-free union-find where that pass would count.
 *   root_dev    : n int32, required.  root[i] = the smallest index in i's component, so root[i] == i marks one representative per cluster.
 *                 (It is the union-find's parent array while the call runs.)
 *   cluster_dev : n int32 or NULL.  A dense id in [0, num): clusters are numbered in ascending order of their root.
 *   size_dev    : n int32 or NULL.  The number of spheres in i's cluster, written for every member.
 *   num_dev     : 1 int64 or NULL (4-byte alignment suffices).  The number of clusters.
 * Integers only, and the same answer whatever the interleaving of the lanes: a tree's final root is its smallest index.  Indices are into
 * L: rt_prepared_get_sphere_ids maps them to the caller's order.  A scene of one sphere gives root = {0}, num = 1.
 * Enqueued on the context's stream (completion: rt_context_sync).  Scratch for the ids and the count is cached on the context (the range
 * queries' buffer, grown on demand).  Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device
 * context, NULL root_dev, a margin outside [0, 1e9] or not finite (-0.0 counts as 0).  rt_context_last_launch: "family=clusters". */
int rt_contact_clusters(rt_context *ctx, const rt_prepared *ps, float margin, int32_t *root_dev, int32_t *cluster_dev, int32_t *size_dev,
                        int64_t *num_dev);
/* ---- box queries: EVERY sphere that meets a caller-supplied axis-aligned box, with no cap ---------------------------------------------
 * A query is a box {lo.xyz, hi.xyz} and a margin.  boxes6_dev: n x 6 float32 in the context's device memory, rows of 24 bytes; only 4-byte
 * alignment is assumed.  For sphere j of L (centre c, radius r) the gap is the signed distance from the box to the sphere's surface, in
 * exactly this float32 arithmetic (no contraction, correctly rounded sqrtf):
 *   ex = fmaxf(fmaxf(lo.x - c.x, c.x - hi.x), 0.0f);   ey, ez likewise;   gap = sqrtf((ex*ex + ey*ey) + ez*ez) - r
 * Sphere j is selected iff gap <= margin -- and, where first_dev is given, j >= first_dev[i].  Margin 0 is the exact closed sphere / box
 * overlap test: tangency (gap == 0) is selected; it is not the overlap of the sphere's own bounding box with the box.  A sphere whose
 * centre lies inside the box has gap -r.  Brute force over all spheres defines the answer; no tree, builder or variant enters it.
 * IDENTITY: with lo == hi == p the expression is rt_nearest_spheres's gap of the point p, bit for bit (the excess of an axis is |fl(p - c)|),
 * so a degenerate box reproduces rt_spheres_within_* at p with max_dist = margin exactly: offsets, index and gap bits.
 * A box is valid iff its six components are finite and lo_k <= hi_k for every k; zero extent in any or all axes is valid.  A per-box margin
 * follows the per-point bounds' rule: NaN, +-inf, negative or above 1e9 is invalid, -0.0 behaves as 0.0.  An invalid box or margin gives an
 * empty row.  Exact for scenes whose spheres are finite with radius >= 0; for other scenes unspecified, but nothing is read or written out of
 * range.
 * The output is rt_spheres_within_count / _fill's, with the same two-phase protocol: offsets (n + 1 int64), then index (int32, ASCENDING j
 * within a row), gap (float32) and point (int32, the row number of each entry: the COO form); any of the last three may be NULL, not all.
 * _fill writes entry offsets[i] + rank only below offsets[i + 1] and below capacity: negative or foreign offsets never cause a write outside
 * [0, capacity).  margin_dev == NULL: the scalar margin for every box; otherwise n float32, one margin per box, and the scalar is ignored.
 * first_dev: as for rt_spheres_within_*.
 * Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device context, n < 0 or n >= 2^31, NULL
 * boxes6_dev, NULL offsets_dev, a negative capacity, every output NULL, a scalar margin (when it is used) outside [0, 1e9] or not finite.
 * n == 0 succeeds and _count still writes offsets_dev[0] = 0.  One lane per box under every variant; rt_context_last_launch:
 * "family=boxes count" / "family=boxes fill", then " (per-box)" with margin_dev, " first" with first_dev. */
int rt_spheres_in_boxes_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *boxes6_dev, float margin,
                              const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev);
int rt_spheres_in_boxes_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *boxes6_dev, float margin,
                             const float *margin_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                             int32_t *index_dev, float *gap_dev, int32_t *point_dev);
/* ---- plane-set queries: EVERY sphere inside a caller-supplied frustum or convex polytope, with no cap --------------------------------
 * A query is nplanes planes and a margin; 1 <= nplanes <= 8, the same for every query of a call (a query that needs fewer repeats a plane:
 * a repeated plane changes nothing).  planes4_dev: n x nplanes x 4 float32 in the context's device memory, rows {a, b, c, d} of 16 bytes;
 * only 4-byte alignment is assumed.  The INSIDE of a plane is a x + b y + c z + d >= 0: normals point inward.  A frustum or a box is six
 * planes; eight leave room for a clipped frustum or a portal.  Each plane is normalised once per query, and for sphere j of L (centre c,
 * radius r) the gap is, in exactly this float32 arithmetic (no contraction, correctly rounded sqrtf and /):
 *   len = sqrtf((a*a + b*b) + c*c);   nx = a/len; ny = b/len; nz = c/len; w = d/len
 *   depth_k = ((nx*c.x + ny*c.y) + nz*c.z) + w                                                  for plane k
 *   gap = fmaxf(fmaxf(... fmaxf(0.0f, -depth_0) ..., -depth_{K-2}), -depth_{K-1}) - r           (planes in the caller's order)
 * Sphere j is selected iff gap <= margin -- and, where first_dev is given, j >= first_dev[i].  At margin 0 that is exactly "the closed ball
 * meets every closed half-space", the standard frustum-culling test.  It is CONSERVATIVE for the polytope itself: a sphere outside an edge
 * or a corner of it can be selected; a sphere that meets the polytope is never dropped.  A centre inside every half-space has gap -r.
 * Brute force over all spheres defines the answer; no tree, builder or variant enters it.
 * A plane is valid iff a, b, c, d are finite, 2^-40 <= len <= 2^40 and the four quotients are finite.  A per-query margin follows the box
 * queries' rule: NaN, +-inf, negative or above 1e9 is invalid, -0.0 behaves as 0.0.  A query with an invalid plane or margin gives an empty
 * row.  Exact for scenes whose spheres are finite with radius >= 0; for other scenes unspecified, but nothing is read or written out of range.
 * RELATION TO THE BOX QUERIES: a box {lo, hi} written as the six planes (1,0,0,-lo.x), (0,1,0,-lo.y), (0,0,1,-lo.z), (-1,0,0,hi.x),
 * (0,-1,0,hi.y), (0,0,-1,hi.z) has len exactly 1, and every -depth is rt_spheres_in_boxes_*'s per-axis excess, bit for bit.  So the plane
 * gap is <= the box gap for every sphere -- the plane row is a superset of the box row -- and where at most one axis has a positive excess e
 * the two gaps are equal in every bit (sqrtf(fl(e*e)) == e).
 * The output is rt_spheres_in_boxes_count / _fill's, with the same two-phase protocol: offsets (n + 1 int64), then index (int32, ASCENDING j
 * within a row), gap (float32) and point (int32, the row number of each entry: the COO form); any of the last three may be NULL, not all.
 * _fill writes entry offsets[i] + rank only below offsets[i + 1] and below capacity: negative or foreign offsets never cause a write outside
 * [0, capacity).  margin_dev == NULL: the scalar margin for every query; otherwise n float32, one margin per query, and the scalar is
 * ignored.  first_dev: as for rt_spheres_within_*.
 * Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device context, n < 0 or n >= 2^31, nplanes < 1
 * or nplanes > 8, NULL planes4_dev, NULL offsets_dev, a negative capacity, every output NULL, a scalar margin (when it is used) outside
 * [0, 1e9] or not finite.  n == 0 succeeds and _count still writes offsets_dev[0] = 0.  One lane per query under every variant;
 * rt_context_last_launch: "family=planes count k=K" / "family=planes fill k=K", then " (per-query)" with margin_dev, " first" with first_dev. */
int rt_spheres_in_planes_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *planes4_dev, int32_t nplanes, float margin,
                               const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev);
int rt_spheres_in_planes_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *planes4_dev, int32_t nplanes, float margin,
                              const float *margin_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                              int32_t *index_dev, float *gap_dev, int32_t *point_dev);
/* ---- along-ray queries: EVERY sphere a ray crosses, or a moving sphere touches, over its whole interval, with no cap ---------------------
 * rt_multi_hit_rays and rt_sweep_spheres return the first k <= 32 crossings or contacts and an uncapped count; these entries return the rest.
 * A query is a ray {o, d} (rays_dev: the n x 6 float32 layout of the ray queries), a radius rq and an interval (t_min, t_max); optionally an
 * excluded index (rt_sweep_spheres_ranged's rule) and a lower index bound `first` (rt_spheres_within_*'s rule).
 * SELECTION: rt_sweep_spheres's rule, unchanged.  Sphere j of L is selected for query i iff
 *   - it is consulted: every inner node on its root path passes aabb_hit over (t_min, t_max) on the node's box widened by rq per component,
 *     fl(lo_k - rq) and fl(hi_k + rq);
 *   - the contact rule above gives a contact (an entry contact or an overlap at the start) against (c, R = r + rq);
 *   - j != exclude_dev[i] (exclude_dev given; a value no sphere has excludes nothing);
 *   - j >= first_dev[i] (first_dev given; <= 0 selects from 0, >= the sphere count gives an empty row; a compare at the leaf, no pruning).
 * There is no k.  Like the sweep's, the answer is defined by the tree: on a tree taller than the AABB propagation's floor(log2 n) + 2 sweeps
 * the partial boxes nearest the root enter it.
 * OUTPUT: CSR, in rt_spheres_within_count / _fill's two phases (count and scan, read offsets_dev[n], allocate, fill with the SAME query):
 *   offsets : n + 1 int64; offsets[0] = 0, offsets[n] the total.
 *   index   : total int32; row i at [offsets[i], offsets[i + 1]), in ASCENDING j -- not by tau.
 *   roots   : total x 2 float32, rows {t1, t2}: the two roots of sphere_hit against (c, R), exactly the values the contact rule compared,
 *             UNCLAMPED -- t1 may lie before t_min, t2 past t_max.  Written as one 8-byte store per row; 4-byte alignment suffices.
 *   start   : total uint8; 0 an entry contact (tau = t1), 1 an overlap at the start (tau = t_min + 0.0f).
 *   query   : total int32, the row number i of each entry (the COO form).
 * Any of the four entry arrays may be NULL, not all.  _fill writes entry offsets[i] + rank only below offsets[i + 1] and below capacity, and
 * nothing for a negative offsets[i]: foreign offsets never cause a write outside [0, capacity).
 * PER-QUERY VALUES: radius_dev == NULL: the scalar radius for every query; otherwise n float32 and the scalar is ignored.  t_min_dev and
 * t_max_dev: both NULL (the scalar pair for every query) or both given (n float32 each; the scalar pair is ignored).  A per-query interval
 * that fails 0 <= t_min <= t_max <= 1e9 or radius that fails 0 <= radius <= 1e9 (NaN, +-inf included) gives an empty row, its walk does not
 * start; -0.0 behaves as +0.0.
 * IDENTITIES (each follows from the shared rule):
 *   1. Without first_dev, row i's length is rt_sweep_spheres_ranged's count_dev[i] for the same query.
 *   2. A row with count <= 32, ordered by (tau, j) with tau = start ? t_min + 0.0f : t1, is rt_sweep_spheres's index, start and
 *      hit7[.., 0], bit for bit.
 *   3. At rq = 0 the consulted leaves are rt_multi_hit_rays's and R = r + 0 is r.  The roots of a row's entries that lie strictly inside
 *      (t_min, t_max), ordered by (t, j, root): their number is rt_multi_hit_rays's count, and the first min(count, 32) are its index, root
 *      and hit7[.., 0], bit for bit.  The selected set is a SUPERSET of the crossed spheres: a segment wholly inside a sphere is selected
 *      (an overlap at the start) with no root inside the interval.
 * Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device context, n < 0 or n >= 2^31, NULL
 * rays_dev, NULL offsets_dev, a negative capacity, every output NULL, exactly one of t_min_dev / t_max_dev NULL, a scalar interval (when it
 * is used) that fails the rule, a scalar radius (when it is used) outside [0, 1e9] or not finite.  n == 0 succeeds and _count still writes
 * offsets_dev[0] = 0.  One lane per query under every variant; rt_context_last_launch: "family=along count" / "family=along fill", then
 * " (per-query)" with any of radius_dev, t_min_dev, t_max_dev, " exclude" with exclude_dev, " first" with first_dev. */
int rt_spheres_along_rays_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius,
                                const float *radius_dev, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev,
                                const int32_t *exclude_dev, const int32_t *first_dev, int64_t *offsets_dev);
int rt_spheres_along_rays_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius,
                               const float *radius_dev, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev,
                               const int32_t *exclude_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                               int32_t *index_dev, float *roots_dev, uint8_t *start_dev, int32_t *query_dev);
/* ---- visibility matrices: EVERY point against EVERY target or direction, one bit per pair, with no n x m ray buffer ---------------------
 * n shading points against m lights, n sensors against m landmarks, n surface points against a fan of m hemisphere directions: a PRODUCT
 * of queries.  Through rt_occluded_rays it needs n * m * 24 bytes of rays in device memory; here each pair's ray is made in registers.
 * points3_dev: n x 3 float32.  targets3_dev: m x 3 float32, positions (RT_PAIRS_TARGETS) or directions (RT_PAIRS_DIRECTIONS).  Both need
 * only 4-byte alignment (the rows are 12 bytes).
 * DEFINITION, in binary32 without contraction.  Pair (i, j) has the ray o = P_i and
 *   RT_PAIRS_TARGETS    : d = (fl(T_j.x - P_i.x), fl(T_j.y - P_i.y), fl(T_j.z - P_i.z));
 *   RT_PAIRS_DIRECTIONS : d = T_j.
 * The pair is VALID iff all six components of o and d are finite and d is not (+-0, +-0, +-0).  It is VISIBLE iff it is valid and
 * rt_occluded_rays on that ray over (t_min, t_max) gives 0: no leaf whose every inner ancestor passes aabb_hit over (t_min, t_max) has a
 * root strictly inside the interval.  An invalid pair is not visible and its walk does not start: a point equal to its target, any pair
 * of a NaN point, an infinite target, a zero direction.  A shadow test is RT_PAIRS_TARGETS over (eps, 1); ambient occlusion is
 * RT_PAIRS_DIRECTIONS over (eps, radius).
 * OUTPUT (either may be NULL, not both):
 *   visible_dev : n x W uint64, W = (m + 63) / 64, 8-byte aligned.  Bit j & 63 of word visible[i * W + (j >> 6)] is 1 iff pair (i, j) is
 *                 visible; bits j >= m of a row's last word are 0.  The words are the device's little-endian 64-bit integers, so byte b of a
 *                 row holds pairs 8 b .. 8 b + 7, lowest bit first: in Python, a uint8 view of the words through
 *                 numpy.unpackbits(..., bitorder="little") is the n x 64 W matrix.
 *   count_dev   : n int32, the number of set bits of row i.  Exact and the same on every call: an integer sum.
 * Refused (non-zero, rt_last_error set, nothing launched or written): a null scene, a multi-device context, n < 0 or n >= 2^31, m < 1 or
 * m > 2^24, n * W >= 2^31, NULL points3_dev or targets3_dev, both outputs NULL, a mode other than the two, an interval that fails
 * rt_occluded_rays's rule (0 <= t_min <= t_max <= 1e9, both finite).  n == 0 succeeds without a launch ("family=none (no points)").
 * Enqueued on the context's stream (completion: rt_context_sync); count_dev may be zeroed on the stream ahead of the kernel, so it must not
 * be in use by work on another stream.  The same kernels under every variant: a wave owns one point and a run of consecutive words of its
 * row, or, for m <= 32, the whole rows of 64 / G consecutive points (G the least power of two >= m).
 * rt_context_last_launch: "family=pairs targets" or "family=pairs directions", then " mask" with visible_dev and " count" with count_dev.
 * rt_visible_pairs_shaped: the same answer, bit for bit, with the caller's launch shape -- words_per_wave, the number of consecutive words
 * of a row that one wave owns, one point per wave: 0 (the library's rule, which is what rt_visible_pairs runs) or positive (above W: the
 * whole row); negative is refused.  A positive value is appended to the launch string as " words/wave=<K>". */
enum { RT_PAIRS_TARGETS = 0, RT_PAIRS_DIRECTIONS = 1 };
int rt_visible_pairs(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, int64_t m, const float *targets3_dev,
                     int32_t mode, float t_min, float t_max, uint64_t *visible_dev, int32_t *count_dev);
int rt_visible_pairs_shaped(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, int64_t m,
                            const float *targets3_dev, int32_t mode, float t_min, float t_max, uint64_t *visible_dev, int32_t *count_dev,
                            int32_t words_per_wave);
/* ---- sphere groups: 32-bit masks that filter rays and proximity queries ------------------------------------------------------------------
 * Shadow rays that ignore the light's own geometry, picking among selectable objects, collision layers, neighbours of one species, probes that
 * see static but not dynamic bodies: a prepared scene may carry ONE uint32 group word per sphere, and every masked query takes a uint32 mask.
 * RULE: query i sees sphere j iff (groups[j] & mask_i) != 0, an unsigned test -- bit 31 is a bit like the others.  Mask 0 sees nothing: its
 * walk does not start and it gets the entry's miss, empty row or zero count.
 * GROUPS: rt_prepared_set_groups takes n device words in the CALLER's sphere order -- the order rt_prepared_get_sphere_ids maps back to, not
 * L's -- and n must equal rt_prepared_num_spheres.  groups_dev == NULL: the scene has no groups again (their memory is released; n is not
 * looked at).  A scene has no groups until they are set, and a masked entry on such a scene fails with a message that names
 * rt_prepared_set_groups.  Groups survive rt_prepared_update_spheres: sphere c of the caller's order keeps word c wherever the rebuild puts it
 * in L (the first masked entry or rt_prepared_get_groups behind an update derives the words again for the new tree, on the context's stream,
 * ahead of its own work).  Only through the context that prepared the scene, and not through a multi-device context; this holds for every
 * entry of this section.  The words are copied on the context's stream: groups_dev may be reused once that copy has run.
 * rt_prepared_get_groups: groups_dev gets n words in L order (groups_dev[i] belongs to L[i]), node_groups_dev n - 1 words, the exact OR of the
 * group words of every leaf below inner node v, v as rt_prepared_get_bvh numbers the inner nodes; either may be NULL, not both.  Enqueued on
 * the context's stream like rt_prepared_get_sphere_ids (completion: rt_context_sync).
 * ANSWERS.  The ray entries: the unmasked entry's own definition with every unseen sphere treated as absent at the leaf -- rt_intersect_rays'
 * fold over the spheres the tree walk visits, every inner box tested with the caller's interval as there, restricted to the seen spheres, with
 * the same (t, index) tie rule, the same re-intersection and bit-identical {t, p, normal}; occlusion is the OR over the same set.  These are
 * the TREE's answers, as the unmasked ones are -- not those of a scene rebuilt from the seen spheres, which has other boxes and another
 * Morton order.  The proximity entries: the unmasked query's definition over the seen spheres only; the gap bits, the (gap, index) order, the
 * count, the CSR row order and the `first` rule are unchanged, and indices still are indices into the whole of L.
 * The walks skip an inner node whose word shares no bit with the mask.  That is an optimisation, never part of a definition: the word is the
 * exact OR of the leaves below, so a skipped subtree holds only unseen spheres.
 * ARGUMENTS: mask_dev == NULL: the scalar `mask` for every query; otherwise n 4-byte-aligned uint32 in device memory, query i's own, and the
 * scalar is ignored.  The other optional per-query arrays follow rt_spheres_along_rays_*: a NULL pointer means the scalar next to it is used
 * and is checked on the host by the unmasked entry's rule; a given pointer means the scalar is ignored and an invalid per-query value makes
 * that query a miss (an empty row, a zero count) by the kernels' rules.  t_min_dev and t_max_dev come together or not at all.  Every other
 * argument keeps the meaning, limits and refusals of the unmasked entry it mirrors: k <= 32, count_dev == NULL selects the pruned k-nearest
 * walk, the CSR two-pass protocol with its capacity guard (foreign offsets can misplace entries, never put one outside the caller's arrays),
 * n == 0 as there.  One lane per ray or point under every variant. */
int rt_prepared_set_groups(rt_context *ctx, rt_prepared *ps, const uint32_t *groups_dev, int64_t n);
int rt_prepared_get_groups(rt_context *ctx, const rt_prepared *ps, uint32_t *groups_dev, uint32_t *node_groups_dev);
int rt_intersect_rays_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                             const float *t_min_dev, const float *t_max_dev, uint32_t mask, const uint32_t *mask_dev, int32_t *index_dev,
                             float *hit7_dev);
int rt_occluded_rays_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                            const float *t_min_dev, const float *t_max_dev, uint32_t mask, const uint32_t *mask_dev, uint8_t *occluded_dev);
int rt_nearest_spheres_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                              const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, int32_t k, int32_t *count_dev,
                              int32_t *index_dev, float *gap_dev);
int rt_spheres_within_masked_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                   const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, const int32_t *first_dev,
                                   int64_t *offsets_dev);
int rt_spheres_within_masked_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                  const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, const int32_t *first_dev,
                                  const int64_t *offsets_dev, int64_t capacity, int32_t *index_dev, float *gap_dev, int32_t *point_dev);
/* ids_dev: n int32 in the context's device memory; ids_dev[i] = the caller's index of L[i]: the position in spheres7 given to
 * rt_scene_from_spheres / rt_prepare_scene_device / the last rt_prepared_update_spheres, or in the generator's output for rt_scene_rgbbox /
 * _irreg / _floor.  The Morton sort is stable, so both builders (option gpu_build) give the same ids, ascending within a run of equal keys.
 * Enqueued on the context's stream (completion: rt_context_sync). */
int rt_prepared_get_sphere_ids(rt_context *ctx, const rt_prepared *ps, int32_t *ids_dev);
/* The primary rays rt_render_image would trace (get_ray at pixel_u / pixel_v), row-major from the top row: h * w x 6
 * float32 at rays_dev.  cam12 == NULL: the prepared camera.  rt_context_last_launch: "family=camera-rays". */
int rt_camera_rays(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, const float cam12[12], float *rays_dev);

/* ---- device buffers for hosts that have no allocator of their own (the C harness) -- */
int rt_device_alloc(rt_context *ctx, void **out_dev, int64_t bytes);
int rt_device_free(rt_context *ctx, void *dev);
int rt_copy_to_host(rt_context *ctx, void *dst_host, const void *src_dev, int64_t bytes);  /* synchronous */
int rt_copy_to_device(rt_context *ctx, void *dst_dev, const void *src_host, int64_t bytes);  /* synchronous */

#ifdef __cplusplus
}
#endif
#endif
