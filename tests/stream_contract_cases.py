"""Which C entry points tests/test_gpu_stream_contract.py captures and replays, as plain data (no device, no torch): case name
-> the entry points its captured sequence calls.  tests/test_stream_contract_host.py holds this table against the functions
include/lotus_hip.h declares: every one is captured by a case here or excluded below, with the reason."""

FLAT_ROUTES = ["stream-2blocks", "stream-seeded", "stream-siblings", "rq-2groups", "join-ragged-tail", "join-solo", "list-k15",
               "list-split", "list-seeded", "passes-57", "two-phase-k57", "k-beyond-nb"]
IVF_KINDS = ["lvs_ivf_search", "lvs_ivf_sq8_search", "lvs_ivf_pq_search"]

CASES = {
    **{f"flat/{name}": ("lvs_flat_search_keys",) for name in FLAT_ROUTES},
    "flat/seeded": ("lvs_flat_search_seed_scores", "lvs_flat_search_keys_seeded"),
    "flat/hi": ("lvs_flat_search_keys_hi",),
    "flat/hi_banded": ("lvs_flat_search_keys_hi_banded",),
    "flat/fallback": ("lvs_flat_search_keys",),
    "chain/certified": ("lvs_flat_search_keys_hi_banded", "lvs_rescore_keys", "lvs_sort_keys_desc", "lvs_certify_topk_banded",
                        "lvs_certify_topk"),
    "chain/nearest3": ("lvs_nearest3", "lvs_nearest3_select", "lvs_resolve_pairs"),
    "chain/nearest_hi": ("lvs_nearest_hi", "lvs_margin_select", "lvs_margin_select_stats"),
    "merge_keys/7x33x10": ("lvs_merge_keys",),
    "merge_keys/20x3x300": ("lvs_merge_keys",),
    "sort_rows_desc": ("lvs_sort_rows_desc",),
    "keys_to_result": ("lvs_keys_to_result",),
    "scores": ("lvs_scores",),
    "range_join/plain": ("lvs_range_join",),
    "range_join/self": ("lvs_range_join",),
    **{f"pack/d{d}": ("lvs_pack_rows", "lvs_pack_rows_checked", "lvs_absmax", "lvs_gather_rows", "lvs_gather_f32",
                      "lvs_unpack_rows") for d in (100, 200)},
    "ivf/build_lists": ("lvs_ivf_build_lists",),
    **{f"ivf/{kind}/nprobe{nprobe}": (kind + "_keys", kind + "_keys_sel") for kind in IVF_KINDS for nprobe in (1, 16)},
    "ivf/encode": ("lvs_ivf_sq8_encode", "lvs_ivf_pq_encode"),
    "ivf/range_search": ("lvs_ivf_range_search",),
    "ivf/refine_keys": ("lvs_refine_keys",),
    "ivf/recall": ("lvs_keys_overlap", "lvs_ivf_row_lists", "lvs_ivf_probe_ranks"),
    "kmeans/accumulate": ("lvs_kmeans_accumulate", "lvs_kmeans_accumulate_keys"),
    "kmeans/objective": ("lvs_kmeans_objective", "lvs_kmeans_pack_centroids"),
    "kmeans/update_centroids": ("lvs_kmeans_update_centroids",),
    "kmeans/bounds": ("lvs_kmeans_centroid_shift", "lvs_kmeans_bounds_set", "lvs_kmeans_bounds_fix", "lvs_kmeans_bounds_step"),
    "search_sharded": ("lvs_search_sharded",),
}

HOST_ONLY = "host-only: touches no stream"
EXCLUDED = {
    **{name: HOST_ONLY for name in (
        "lvs_abi_version", "lvs_last_error", "lvs_build_flags", "lvs_device_count", "lvs_device_info", "lvs_packed_ld",
        "lvs_flat_search_seed_tiles", "lvs_nearest_bound_coef", "lvs_flat_search_workspace_bytes", "lvs_search_sharded_workspace_bytes",
        "lvs_sort_rows_workspace_bytes", "lvs_nearest_hi_workspace_bytes", "lvs_nearest3_workspace_bytes",
        "lvs_kmeans_accumulate_workspace_bytes", "lvs_kmeans_objective_workspace_bytes", "lvs_kmeans_iteration_workspace_bytes",
        "lvs_ivf_build_workspace_bytes", "lvs_ivf_search_workspace_bytes", "lvs_ivf_range_workspace_bytes",
        "lvs_ivf_sq8_search_workspace_bytes", "lvs_ivf_pq_search_workspace_bytes", "lvs_rand_perm_host",
        "lvs_rand_perm_prefix_host", "lvs_kmeans_split_clusters_host", "lvs_rccl_available", "lvs_rccl_bind",
        "lvs_rccl_bind_all_reduce", "lvs_timing_enable", "lvs_timing_read", "lvs_timing_read_calls")},
    # the header's one exception ("THE ONE ENTRY POINT THAT SYNCHRONISES `stream`"): test_kmeans_iteration_orders_its_launches
    "lvs_kmeans_iteration": "synchronises by contract",
    "lvs_search_sharded_rccl": "needs a communicator",
    "lvs_kmeans_iteration_rccl": "needs a communicator (and synchronises by contract)",
}
