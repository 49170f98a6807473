"""ctypes loader for libray_mi355x.so (the HIP library; include/rt_mi355x.h, include/ray.h).

There is deliberately no fallback: if the shared library is missing or cannot be loaded the
import of this module raises, and if no HIP device is usable Context() raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libray_mi355x.so"
LIB_PATH = os.path.join(HERE, LIB_NAME)

# every symbol include/rt_mi355x.h declares
RT_SYMBOLS = [
    "rt_context_create", "rt_device_count", "rt_context_create_multi", "rt_context_num_devices", "rt_context_gather_mode", "rt_context_rccl_ranks",
    "rt_context_destroy", "rt_last_error", "rt_context_last_launch", "rt_context_entry_counts", "rt_context_entry_info", "rt_context_exit_info", "rt_context_wide_info", "rt_context_sync", "rt_context_set_variant",
    "rt_context_set_option", "rt_context_device_info",
    "rt_scene_rgbbox", "rt_scene_irreg", "rt_scene_floor", "rt_scene_from_spheres", "rt_scene_num_spheres",
    "rt_scene_free",
    "rt_prepare_scene", "rt_prepared_free", "rt_prepared_num_spheres", "rt_prepared_height", "rt_prepared_get_bvh",
    "rt_prepared_get_camera", "rt_prepare_scene_device", "rt_prepared_update_spheres",
    "rt_render", "rt_render_part", "rt_render_image", "rt_render_batch", "rt_render_part_inplace", "rt_ipc_export", "rt_ipc_import", "rt_ipc_close", "rt_part_rows", "rt_place_part", "rt_place_parts", "rt_place_parts_strided", "rt_place_parts_batch", "rt_render_stats", "rt_render_trace",
    "rt_render_timed",
    "rt_trace_rays", "rt_intersect_rays", "rt_occluded_rays", "rt_intersect_rays_ranged", "rt_occluded_rays_ranged",
    "rt_multi_hit_rays", "rt_multi_hit_rays_ranged", "rt_sweep_spheres", "rt_sweep_spheres_ranged", "rt_trace_paths", "rt_trace_paths_shaped", "rt_nearest_spheres", "rt_nearest_spheres_ranged", "rt_prepared_get_sphere_ids",
    "rt_spheres_within_count", "rt_spheres_within_fill", "rt_contact_pairs_count", "rt_contact_pairs_fill", "rt_contact_clusters",
    "rt_spheres_in_boxes_count", "rt_spheres_in_boxes_fill",
    "rt_spheres_in_planes_count", "rt_spheres_in_planes_fill",
    "rt_spheres_along_rays_count", "rt_spheres_along_rays_fill",
    "rt_visible_pairs", "rt_visible_pairs_shaped",
    "rt_prepared_set_groups", "rt_prepared_get_groups", "rt_intersect_rays_masked", "rt_occluded_rays_masked", "rt_nearest_spheres_masked",
    "rt_spheres_within_masked_count", "rt_spheres_within_masked_fill",
    "rt_camera_rays",
    "rt_device_alloc", "rt_device_free", "rt_copy_to_host", "rt_copy_to_device",
]
# every symbol include/ray.h declares (the Futhark-shaped drop-in boundary)
FUTHARK_SYMBOLS = [
    "futhark_context_config_new", "futhark_context_config_free", "futhark_context_config_set_debugging",
    "futhark_context_config_set_logging", "futhark_context_config_set_profiling",
    "futhark_context_config_set_device", "futhark_context_config_set_num_threads", "futhark_context_config_set_cache_file",
    "futhark_context_new", "futhark_context_free", "futhark_context_get_error", "futhark_context_sync",
    "futhark_context_report", "futhark_context_clear_caches", "futhark_context_pause_profiling",
    "futhark_context_unpause_profiling",
    "futhark_entry_rgbbox", "futhark_entry_irreg", "futhark_entry_prepare_scene", "futhark_entry_render",
    "futhark_values_i32_2d", "futhark_free_i32_2d", "futhark_shape_i32_2d", "futhark_new_i32_2d", "futhark_values_raw_i32_2d",
    "futhark_free_opaque_prepared_scene", "futhark_free_opaque_scene",
]


def _load():
    # When torch is installed, import it FIRST: it ships its own libamdhip64.so.7 and the
    # process must have exactly one HIP runtime (ours resolves to the already-loaded soname).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP library first (`make` at the repo root, or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). raytracers_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pf = C.POINTER(C.c_float)
    sig = {
        "rt_context_create": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.c_int]),
        "rt_device_count": (C.c_int, []),
        "rt_context_create_multi": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]),
        "rt_context_num_devices": (C.c_int, [vp]),
        "rt_context_gather_mode": (C.c_char_p, [vp]),
        "rt_context_rccl_ranks": (C.c_int, [vp]),
        "rt_context_destroy": (None, [vp]),
        "rt_last_error": (C.c_char_p, [vp]),
        "rt_context_last_launch": (C.c_char_p, [vp]),
        "rt_context_entry_counts": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(i64), C.POINTER(C.c_uint64), i64]),
        "rt_context_entry_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "rt_context_exit_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "rt_context_wide_info": (C.c_int, [vp, C.POINTER(i32)]),
        "rt_context_sync": (C.c_int, [vp]),
        "rt_context_set_variant": (C.c_int, [vp, C.c_int]),
        "rt_context_set_option": (C.c_int, [vp, C.c_char_p, i64]),
        "rt_context_device_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.c_char_p, C.c_int]),
        "rt_scene_rgbbox": (C.c_int, [vp, C.POINTER(vp)]),
        "rt_scene_irreg": (C.c_int, [vp, C.POINTER(vp)]),
        "rt_scene_floor": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_float]),
        "rt_scene_from_spheres": (C.c_int, [vp, C.POINTER(vp), vp, i64, pf, pf, C.c_float]),
        "rt_scene_num_spheres": (i64, [vp]),
        "rt_scene_free": (C.c_int, [vp, vp]),
        "rt_prepare_scene": (C.c_int, [vp, C.POINTER(vp), i64, i64, vp]),
        "rt_prepared_free": (C.c_int, [vp, vp]),
        "rt_prepared_num_spheres": (i64, [vp]),
        "rt_prepared_height": (i32, [vp]),
        "rt_prepared_get_bvh": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt_prepared_get_camera": (C.c_int, [vp, vp, vp]),
        "rt_prepare_scene_device": (C.c_int, [vp, C.POINTER(vp), i64, i64, vp, i64, pf, pf, C.c_float]),
        "rt_prepared_update_spheres": (C.c_int, [vp, vp, vp, i64]),
        "rt_render": (C.c_int, [vp, vp, i64, i64, vp]),
        "rt_render_part": (C.c_int, [vp, vp, i64, i64, i32, i32, i32, i32, vp]),
        "rt_render_image": (C.c_int, [vp, vp, i64, i64, vp, i32, i32, i32, i32, vp]),
        "rt_render_batch": (C.c_int, [vp, vp, i64, i64, i32, i32, i32, i32, i32, vp, i64, vp]),
        "rt_render_part_inplace": (C.c_int, [vp, vp, i64, i64, i32, i32, i32, i32, i32, vp, i64, vp]),
        "rt_ipc_export": (C.c_int, [vp, vp, vp]),
        "rt_ipc_import": (C.c_int, [vp, vp, C.POINTER(vp)]),
        "rt_ipc_close": (C.c_int, [vp, vp]),
        "rt_part_rows": (i64, [i64, i32, i32, i32]),
        "rt_place_part": (C.c_int, [vp, i64, i64, i32, i32, i32, vp, vp]),
        "rt_place_parts": (C.c_int, [vp, i64, i64, i32, i32, i64, vp, vp]),
        "rt_place_parts_strided": (C.c_int, [vp, i64, i64, i32, i32, i64, vp, vp]),
        "rt_place_parts_batch": (C.c_int, [vp, i64, i64, i32, i32, i64, i32, i64, i64, vp, vp]),
        "rt_render_stats": (C.c_int, [vp, vp, i64, i64, i32, vp]),
        "rt_render_trace": (C.c_int, [vp, vp, i64, i64, i32, vp, i32, C.POINTER(i32)]),
        "rt_render_timed": (C.c_int, [vp, vp, i64, i64, i32, i32, i32, i32, vp, i32, i32, vp]),
        "rt_device_alloc": (C.c_int, [vp, C.POINTER(vp), i64]),
        "rt_device_free": (C.c_int, [vp, vp]),
        "rt_copy_to_host": (C.c_int, [vp, vp, vp, i64]),
        "rt_copy_to_device": (C.c_int, [vp, vp, vp, i64]),
        "rt_trace_rays": (C.c_int, [vp, vp, i64, vp, i32, vp, vp]),
        "rt_intersect_rays": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, vp, vp]),
        "rt_occluded_rays": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, vp]),
        "rt_intersect_rays_ranged": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, vp]),
        "rt_occluded_rays_ranged": (C.c_int, [vp, vp, i64, vp, vp, vp, vp]),
        "rt_multi_hit_rays": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, i32, vp, vp, vp, vp]),
        "rt_multi_hit_rays_ranged": (C.c_int, [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp]),
        "rt_sweep_spheres": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, C.c_float, i32, vp, vp, vp, vp]),
        "rt_sweep_spheres_ranged": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
        "rt_trace_paths": (C.c_int, [vp, vp, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "rt_trace_paths_shaped": (C.c_int, [vp, vp, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32]),
        "rt_nearest_spheres": (C.c_int, [vp, vp, i64, vp, C.c_float, i32, vp, vp, vp]),
        "rt_nearest_spheres_ranged": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, vp, vp]),
        "rt_prepared_get_sphere_ids": (C.c_int, [vp, vp, vp]),
        "rt_spheres_within_count": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, vp, vp]),
        "rt_spheres_within_fill": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, vp, vp, i64, vp, vp, vp]),
        "rt_contact_pairs_count": (C.c_int, [vp, vp, C.c_float, vp]),
        "rt_contact_pairs_fill": (C.c_int, [vp, vp, C.c_float, vp, i64, vp, vp]),
        "rt_contact_clusters": (C.c_int, [vp, vp, C.c_float, vp, vp, vp, vp]),
        "rt_spheres_in_boxes_count": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, vp, vp]),
        "rt_spheres_in_boxes_fill": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, vp, vp, i64, vp, vp, vp]),
        "rt_spheres_in_planes_count": (C.c_int, [vp, vp, i64, vp, C.c_int32, C.c_float, vp, vp, vp]),
        "rt_spheres_in_planes_fill": (C.c_int, [vp, vp, i64, vp, C.c_int32, C.c_float, vp, vp, vp, i64, vp, vp, vp]),
        "rt_spheres_along_rays_count": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
        "rt_spheres_along_rays_fill": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
        "rt_visible_pairs": (C.c_int, [vp, vp, i64, vp, i64, vp, i32, C.c_float, C.c_float, vp, vp]),
        "rt_visible_pairs_shaped": (C.c_int, [vp, vp, i64, vp, i64, vp, i32, C.c_float, C.c_float, vp, vp, i32]),
        "rt_prepared_set_groups": (C.c_int, [vp, vp, vp, i64]),
        "rt_prepared_get_groups": (C.c_int, [vp, vp, vp, vp]),
        "rt_intersect_rays_masked": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, vp, vp, C.c_uint32, vp, vp, vp]),
        "rt_occluded_rays_masked": (C.c_int, [vp, vp, i64, vp, C.c_float, C.c_float, vp, vp, C.c_uint32, vp, vp]),
        "rt_nearest_spheres_masked": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, C.c_uint32, vp, i32, vp, vp, vp]),
        "rt_spheres_within_masked_count": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, C.c_uint32, vp, vp, vp]),
        "rt_spheres_within_masked_fill": (C.c_int, [vp, vp, i64, vp, C.c_float, vp, C.c_uint32, vp, vp, vp, i64, vp, vp, vp]),
        "rt_camera_rays": (C.c_int, [vp, vp, i64, i64, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
