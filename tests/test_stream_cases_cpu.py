"""Every device entry point of the C ABI has a case in tests/_stream_cases.py (the table the
ordering tests of tests/test_gpu_stream_order.py run over), or a stated reason for having none."""
import ctypes

from gala import _abi

import _stream_cases as S


def test_every_device_entry_point_has_a_stream_case():
    entries = S.device_entry_points()
    assert len(entries) > 40 and "gala_spmm_f32" in entries and "gala_gat_in_q_scatter_f32" in entries
    # the size queries return a byte or column count, the host functions take no stream
    assert not entries & {"gala_dense_grad_workspace", "gala_gat_in_bwd_workspace", "gala_gat_in_split_ws_cols",
                          "gala_abi_version", "gala_last_hip_error", "gala_status_string"}
    assert not any(n.startswith("gala_host_") for n in entries)
    cases, excluded = set(S.CASES), set(S.EXCLUDED)
    assert not cases & excluded
    missing = entries - cases - excluded
    assert not missing, f"device entry points without a stream case or an exclusion: {sorted(missing)}"
    stale = (cases | excluded) - entries
    assert not stale, f"no such device entry point: {sorted(stale)}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in S.EXCLUDED.values())
    assert set(S.DIRECT) <= cases
    assert all(k.split("-")[0] in cases and k not in cases for k in S.EXTRA_CASES)


def test_a_missing_case_is_noticed():
    """The check above fails when one case leaves the table (or a new ABI function arrives)."""
    entries = S.device_entry_points()
    for name in S.CASES:
        assert entries - (set(S.CASES) - {name}) - set(S.EXCLUDED) == {name}
    sig = dict(_abi.SIGNATURES, gala_new_op_f32=(ctypes.c_int, [ctypes.c_int64, ctypes.c_void_p]))
    new = {n for n, (res, args) in sig.items()
           if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p and not n.startswith("gala_host_")}
    assert new - set(S.CASES) - set(S.EXCLUDED) == {"gala_new_op_f32"}
