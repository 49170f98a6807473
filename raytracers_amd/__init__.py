"""raytracers_amd -- MI355X-native (gfx950) render hot path of athas/raytracers.

The product is libray_mi355x.so (hand-written HIP kernels behind a C ABI; see include/).
This package is the thin host-side mirror of the reference's call surface plus the
row-tile sharding used for multi-GPU renders.  Importing it loads the HIP library and
fails loudly if it has not been built."""
from .api import (Context, Prepared, RtError, Scene, MAX_DEPTH, ROWS_PER_TILE, VARIANT_AUTO, VARIANT_PERSISTENT, VARIANT_POOLED,  # noqa: F401
                  VARIANT_PIXEL, part_rows, place_part, place_parts, place_parts_batch, prepare_scene, prepare_scene_from_spheres, render, render_batch_into, render_image, render_inplace_into, render_into, render_timed,
                  ipc_export, ipc_import, ipc_close, trace_rays, trace_rays_into, intersect_rays, intersect_rays_into, camera_rays,
                  camera_rays_into, occluded_rays, occluded_rays_into, intersect_rays_ranged_into, occluded_rays_ranged_into,
                  multi_hit_rays, multi_hit_rays_into, multi_hit_rays_ranged_into,
                  sweep_spheres, sweep_spheres_into, sweep_spheres_ranged_into,
                  trace_paths, trace_paths_into, PATH_ESCAPED, PATH_ABSORBED, PATH_TRUNCATED,
                  nearest_spheres, nearest_spheres_into, nearest_spheres_ranged_into,
                  spheres_within, spheres_within_count_into, spheres_within_fill_into,
                  spheres_in_boxes, spheres_in_boxes_count_into, spheres_in_boxes_fill_into,
                  spheres_in_planes, spheres_in_planes_count_into, spheres_in_planes_fill_into, frustum_planes, tile_frusta,
                  spheres_along_rays, spheres_along_rays_count_into, spheres_along_rays_fill_into, row_contacts, row_crossings,
                  visible_pairs, visible_pairs_into, unpack_visible, PAIRS_TARGETS, PAIRS_DIRECTIONS,
                  contact_pairs, contact_pairs_count_into, contact_pairs_fill_into,
                  contact_clusters, contact_clusters_into, cluster_members,
                  intersect_rays_masked_into, occluded_rays_masked_into, nearest_spheres_masked_into,
                  spheres_within_masked_count_into, spheres_within_masked_fill_into, nearest_spheres_masked, spheres_within_masked)
