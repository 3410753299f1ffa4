"""CPU: the reference built for gfx950 (oracle/_ref/<kernel>_gfx950.co, oracle/Makefile) has the layout the launcher
(oracle/device_ref.hip) packs. Checked from the metadata sidecars, so it also runs where the reference is absent from the
build (it then skips: there is nothing to check)."""
import pytest

from oracle import oracle

HIDDEN = {f"hidden_{k}_{a}" for k in ("block_count", "group_size", "remainder", "global_offset") for a in "xyz"} | {
    "hidden_grid_dims"}


def _notes(kernel):
    co, notes = oracle.device_code_object(kernel), oracle.device_notes(kernel)
    if not co.exists() or not notes.exists():
        pytest.skip(f"{co.name} not built (the reference was absent at build time)")
    return notes.read_text()


@pytest.mark.parametrize("kernel", list(oracle.KERNELS))
def test_sidecar_matches_the_launcher(kernel):
    text = _notes(kernel)
    oracle.check_device_layout(kernel, text)        # raises on any mismatch
    meta = oracle.parse_notes(text)
    assert meta["target"] == "amdgcn-amd-amdhsa--gfx950" and "xnack+" not in meta["target"]
    (k,) = meta["kernels"]
    assert k["name"] == kernel and k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0
    assert k.get("uses_dynamic_stack") == "false"
    # the only hidden arguments are the code-object-v5 ones the runtime fills for any module launch
    hidden = {a["value_kind"] for a in k["args"] if a["value_kind"].startswith("hidden_")}
    assert hidden <= HIDDEN, hidden - HIDDEN


def test_layout_check_refuses_a_mismatch():
    text = _notes("shade")
    with pytest.raises(ValueError, match="explicit arguments"):
        oracle.check_device_layout("shade", text.replace(".offset:         16", ".offset:         12", 1))
    with pytest.raises(ValueError, match="xnack"):
        oracle.check_device_layout("shade", text.replace("--gfx950", "--gfx950:xnack+"))
    with pytest.raises(ValueError, match="private_segment"):
        oracle.check_device_layout("shade", text.replace("private_segment_fixed_size: 0", "private_segment_fixed_size: 16"))
    with pytest.raises(ValueError, match="one kernel"):
        oracle.check_device_layout("hittest", text)
