"""Every function of include/lotus_hip.h is captured and replayed by a case of tests/test_gpu_stream_contract.py, or is excluded
with a reason (tests/stream_contract_cases.py).  A new entry point fails here until someone decides which it is."""
from lotus_amd import _capi
from stream_contract_cases import CASES, EXCLUDED, FLAT_ROUTES


def test_every_entry_point_is_captured_or_excluded_with_a_reason():
    declared = set(_capi.PROTOTYPES)
    assert len(declared) >= 80 and declared == set(_capi.SIGNATURES), declared ^ set(_capi.SIGNATURES)
    covered = {entry for entries in CASES.values() for entry in entries}
    assert not covered & set(EXCLUDED), covered & set(EXCLUDED)
    assert covered | set(EXCLUDED) == declared, (sorted(declared - covered - set(EXCLUDED)), sorted((covered | set(EXCLUDED)) - declared))
    reasons = ("host-only", "synchronises by contract", "needs a communicator")
    assert all(reason.startswith(reasons) for reason in EXCLUDED.values())
    # an excluded name is what its reason says: the host-only ones take no stream, the others do
    takes_stream = {name for name, p in _capi.PROTOTYPES.items() if "void* stream" in map(" ".join, zip(p.types, p.names))}
    assert {n for n, r in EXCLUDED.items() if r.startswith("host-only")} == declared - takes_stream
    assert covered == takes_stream - {"lvs_kmeans_iteration", "lvs_search_sharded_rccl", "lvs_kmeans_iteration_rccl"}


def test_one_flat_shape_per_route():
    from extent_cases import FLAT, FLAT_BY_NAME

    assert {FLAT_BY_NAME[name].route for name in FLAT_ROUTES} == {c.route for c in FLAT}
