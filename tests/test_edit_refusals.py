"""What the edit-distance C entry points refuse, and in which words (no GPU): the six row entries (statistics, operations and
confusions, uniform and weighted), the two workspace sizes and amx_edit_matrix.  Every call hands over pointers that are never
dereferenced and has exactly one argument wrong, so it returns before any device work; the return code and the whole text of
amx_last_error are pinned.  Which message wins when two arguments are wrong is not part of the contract."""
import ctypes as C
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)  # never dereferenced: every call here is refused, or has no rows

HEAD = ["device", "tokens", "stride_o", "stride_n", "stride_k", "O", "N", "K", "T", "counts", "hyp_counts", "label_offsets",
        "label_ids", "groups", "G", "map_offsets", "map_values", "label_maps", "hyp_maps", "H", "max_expected", "max_actual",
        "workspace", "workspace_bytes"]
OPS_HEAD = [name for name in HEAD if name not in ("stride_k", "K")]
COSTS = ["insertion_cost", "deletion_cost", "cost_tables", "cost_table_data"]
CONFUSION_TAIL = ["best", "table", "capacity", "row_events", "counters", "stream"]
ENTRIES = {
    "amx_edit_statistics": HEAD + ["statistics", "best", "totals", "stream"],
    "amx_edit_operations": OPS_HEAD + ["max_ops", "operations", "operation_counts", "stream"],
    "amx_edit_weighted_statistics": HEAD + COSTS + ["statistics", "best", "totals", "costs", "stream"],
    "amx_edit_weighted_operations": OPS_HEAD + COSTS + ["max_ops", "operations", "operation_counts", "costs", "stream"],
    "amx_edit_confusions": HEAD + CONFUSION_TAIL,
    "amx_edit_weighted_confusions": HEAD + COSTS + CONFUSION_TAIL,
}
WEIGHTED = [name for name in ENTRIES if "weighted" in name]
OPERATIONS = [name for name in ENTRIES if "operations" in name]
CONFUSIONS = [name for name in ENTRIES if "confusions" in name]
WITH_K = [name for name in ENTRIES if name not in OPERATIONS]
MAX_EXPECTED, MAX_ACTUAL = 8, 5
VALUES = {"device": 0, "stride_o": 4, "stride_n": 4, "stride_k": 4, "O": 1, "N": 2, "K": 2, "T": 4, "G": 1, "H": 1,
          "max_expected": MAX_EXPECTED, "max_actual": MAX_ACTUAL, "workspace_bytes": 1 << 20, "insertion_cost": 1.0,
          "deletion_cost": 1.0, "max_ops": MAX_EXPECTED + MAX_ACTUAL, "capacity": 16}
OPTIONAL = ("hyp_counts", "cost_table_data", "stream")  # null in every call; `best` of the confusions too, see below

LENGTHS = "expanded lengths must be 0 to 65535"
COST_LIMITS = "insertion and deletion costs must be finite and above 0"
NULL = "null buffer"
CAPACITY = "a confusion table holds a power of two of 16 to 268435456 slots"
MAX_OPS = {"amx_edit_operations": ("max_ops must be max(max_expected, max_actual) to 2^31 - 1", max(MAX_EXPECTED, MAX_ACTUAL)),
           "amx_edit_weighted_operations": ("max_ops must be max_expected + max_actual to 2^31 - 1", MAX_EXPECTED + MAX_ACTUAL)}


@pytest.fixture(scope="module")
def handle():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib.load()


def pointers(entry):
    """The arguments of `entry` that are pointers, optional ones included."""
    return [name for name in ENTRIES[entry] if name not in VALUES]


def required(entry):
    return [name for name in pointers(entry) if name not in OPTIONAL and not (name == "best" and entry in CONFUSIONS)]


def call(handle, entry, **changes):
    """(return code, amx_last_error) of `entry` with valid arguments but for `changes`."""
    arguments = {name: VALUES.get(name, None if name in OPTIONAL else P) for name in ENTRIES[entry]}
    assert set(changes) <= set(arguments), (entry, changes)
    arguments.update(changes)
    code = getattr(handle, entry)(*(arguments[name] for name in ENTRIES[entry]))
    return code, handle.amx_last_error(None).decode()


def refused(handle, entry, message, **changes):
    from allophant_amd import lib

    assert call(handle, entry, **changes) == (lib.AMX_EINVAL, message), (entry, changes)


def needed(handle, entry, max_expected=MAX_EXPECTED, max_actual=MAX_ACTUAL):
    """The workspace size that `entry` asks for at the default shape, and the name of the call that reports it."""
    size = C.c_size_t()
    rows = VALUES["O"] * VALUES["N"]
    if entry in ("amx_edit_statistics", "amx_edit_weighted_statistics"):
        assert handle.amx_edit_workspace(rows * VALUES["K"], max_expected, max_actual, C.byref(size)) == 0
        return size.value, "amx_edit_workspace"
    assert handle.amx_edit_operations_workspace(rows, max_expected, max_actual, C.byref(size)) == 0
    return size.value, "amx_edit_operations_workspace"


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_geometry_and_limits(handle, entry):
    for name in ("O", "N", "T"):
        refused(handle, entry, "negative edit geometry", **{name: -1})
    for name in ("max_expected", "max_actual"):
        for value in (-1, 65536):
            refused(handle, entry, LENGTHS, **{name: value})
    refused(handle, entry, "at least one group", G=0)
    refused(handle, entry, "H must be 1 or G hypothesis-map sets", G=3, H=2)
    rows = "O * N must stay below 2^31" if entry in OPERATIONS else "O * N * K must stay below 2^31"
    refused(handle, entry, rows, O=65536, N=65536)


@pytest.mark.parametrize("entry", WITH_K)
def test_candidates(handle, entry):
    for K in (0, 65):
        refused(handle, entry, "K must be 1 to 64 candidates", K=K)


@pytest.mark.parametrize("entry", WEIGHTED)
def test_costs(handle, entry):
    for name in ("insertion_cost", "deletion_cost"):
        for value in (0.0, -1.0, math.inf, math.nan):
            refused(handle, entry, COST_LIMITS, **{name: value})


@pytest.mark.parametrize("entry", OPERATIONS)
def test_max_ops(handle, entry):
    """The uniform call's bound is the longer side, the weighted call's the sum; a value at the bound passes (the call is then
    refused for its workspace, which is checked later)."""
    message, bound = MAX_OPS[entry]
    refused(handle, entry, message, max_ops=bound - 1)
    refused(handle, entry, message, max_ops=2 ** 31)
    size, name = needed(handle, entry)
    refused(handle, entry, f"workspace smaller than {name}", max_ops=bound, workspace_bytes=size - 1)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers_and_workspace(handle, entry):
    weighted = ["cost_tables"] if entry in WEIGHTED else []
    assert set(weighted) <= set(required(entry)) and len(required(entry)) >= 12
    for name in required(entry):
        refused(handle, entry, NULL, **{name: None})
    size, name = needed(handle, entry)
    assert size > 0
    refused(handle, entry, f"workspace smaller than {name}", workspace_bytes=size - 1)
    if entry in CONFUSIONS:  # `best` may be null: the call gets as far as the workspace check
        refused(handle, entry, f"workspace smaller than {name}", best=None, workspace_bytes=size - 1)


@pytest.mark.parametrize("entry", CONFUSIONS)
def test_confusion_capacity(handle, entry):
    for capacity in (8, 24, 2 ** 33):
        refused(handle, entry, CAPACITY, capacity=capacity)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_nothing_to_score(handle, entry):
    """No rows: AMX_OK without touching a pointer, whatever the workspace."""
    from allophant_amd import lib

    nulls = {name: None for name in pointers(entry)}
    for empty in ({"O": 0}, {"N": 0}):
        assert call(handle, entry, workspace_bytes=0, **nulls, **empty)[0] == lib.AMX_OK, (entry, empty)


@pytest.mark.parametrize("entry", ["amx_edit_workspace", "amx_edit_operations_workspace"])
def test_workspace_sizes(handle, entry):
    from allophant_amd import lib

    function, size = getattr(handle, entry), C.c_size_t()

    def refused_size(message, *arguments):
        assert function(*arguments) == lib.AMX_EINVAL and handle.amx_last_error(None).decode() == message, arguments

    refused_size("null size pointer", 1, 1, 1, None)
    for rows in (-1, 2 ** 31):
        refused_size("rows must be 0 to 2^31 - 1", rows, 1, 1, C.byref(size))
    for value in (-1, 65536):
        refused_size(LENGTHS, 1, value, 1, C.byref(size))
        refused_size(LENGTHS, 1, 1, value, C.byref(size))
    assert function(0, 0, 0, C.byref(size)) == lib.AMX_OK and size.value == 0
    assert function(2 ** 31 - 1, 1, 1, C.byref(size)) == lib.AMX_OK and size.value > 0


MATRIX = ["device", "expected_offsets", "expected_ids", "actual_offsets", "actual_ids", "rows", "max_expected", "max_actual",
          "insertion_cost", "deletion_cost", "cost_table", "V", "workspace", "workspace_bytes", "matrix", "status", "stream"]


def test_matrix(handle):
    from allophant_amd import lib

    values = {"device": 0, "rows": 3, "max_expected": MAX_EXPECTED, "max_actual": MAX_ACTUAL, "insertion_cost": 1.0,
              "deletion_cost": 1.0, "V": 4, "workspace_bytes": 1 << 20, "stream": None}

    def matrix(**changes):
        arguments = {name: values.get(name, P) for name in MATRIX}
        assert set(changes) <= set(arguments), changes
        arguments.update(changes)
        code = handle.amx_edit_matrix(*(arguments[name] for name in MATRIX))
        return code, handle.amx_last_error(None).decode()

    def refused_matrix(message, **changes):
        assert matrix(**changes) == (lib.AMX_EINVAL, message), changes

    for rows in (-1, 2 ** 31):
        refused_matrix("rows must be 0 to 2^31 - 1", rows=rows)
    for name in ("max_expected", "max_actual"):
        for value in (-1, 65536):
            refused_matrix(LENGTHS, **{name: value})
    for name in ("insertion_cost", "deletion_cost"):
        for value in (0.0, -1.0, math.inf, math.nan):
            refused_matrix(COST_LIMITS, **{name: value})
    for V in (-1, 8193):
        refused_matrix("a cost table covers at most 8192 symbols", V=V)
    for name in ("expected_offsets", "expected_ids", "actual_offsets", "actual_ids", "cost_table", "workspace", "matrix", "status"):
        refused_matrix(NULL, **{name: None})
    size = C.c_size_t()
    assert handle.amx_edit_workspace(values["rows"], MAX_EXPECTED, MAX_ACTUAL, C.byref(size)) == lib.AMX_OK
    refused_matrix("workspace smaller than amx_edit_workspace", workspace_bytes=size.value - 1)
    # without a table (V == 0) `cost_table` may be null: the call gets as far as the workspace check
    refused_matrix("workspace smaller than amx_edit_workspace", V=0, cost_table=None, workspace_bytes=size.value - 1)
    nulls = {name: None for name in MATRIX if name not in values}
    assert matrix(rows=0, workspace_bytes=0, **nulls)[0] == lib.AMX_OK
