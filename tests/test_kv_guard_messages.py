"""CPU: the refusals of the five KV state movers (bitnet_hip_kv_fork_dev, kv_save_dev, kv_restore_dev, kv_shift_dev, kv_permute_dev), pinned by
exact return code and exact message text, and where two refusals apply, by which one is made.  Every call here is refused (or is valid and has
nothing to launch) before anything touches a device.  `{e}` in an expected message is the entry's name without the bitnet_hip_ prefix; the rest
of each message is literal."""
import ctypes as C

import pytest

INVALID = -1  # BITNET_HIP_ERR_INVALID_ARGUMENT
OK = 0
KV_F16 = 2    # BITNET_HIP_ATTN_KV_F16
BIG = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()  # built by __graft_entry__.build() ahead of the suite


@pytest.fixture(scope="module")
def mem():
    buf = (C.c_uint8 * 4096)()
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16  # the buffer (kept alive) and a 16-byte aligned address inside it


# every entry's arguments by name, in the C order; the defaults are a valid call (permute's but for the beam state, which no CPU test can make)
ORDER = {
    "kv_fork_dev": ("src_k", "src_v", "dst_k", "dst_v", "n_layers", "count", "n_kv", "head_dim", "max_pos", "n", "flags", "stream"),
    "kv_save_dev": ("k", "v", "n_layers", "n_kv", "head_dim", "max_pos", "n", "flags", "snap", "stream"),
    "kv_restore_dev": ("snap", "S", "dst_k", "dst_v", "n_layers", "count", "n_kv", "head_dim", "max_pos", "n", "flags", "stream"),
    "kv_shift_dev": ("k", "v", "sin", "cos", "n_layers", "n_kv", "head_dim", "max_pos", "keep", "discard", "n", "flags", "stream"),
    "kv_permute_dev": ("k", "v", "beam", "n_layers", "count", "n_kv", "head_dim", "max_pos", "n", "flags", "stream"),
}
POINTERS = ("src_k", "src_v", "dst_k", "dst_v", "k", "v", "snap", "sin", "cos")
ENTRIES = tuple(ORDER)
COUNTED = {"kv_fork_dev": "n_dst", "kv_restore_dev": "n_dst", "kv_permute_dev": "n_beams"}  # the entries with a destination / beam count
BOUND = {e: "key_bound" if e == "kv_permute_dev" else "n_positions" for e in ENTRIES}          # what each calls its position bound


@pytest.fixture(scope="module")
def refuse(lib, mem):
    """refuse(entry, code, message, **changed arguments): the call returns `code`, and, when refused, leaves exactly `message`"""
    defaults = dict(n_layers=3, count=2, n_kv=2, head_dim=128, max_pos=640, n=10, S=10, keep=2, discard=3, flags=0, stream=None, beam=None)
    defaults.update({name: mem[1] for name in POINTERS})

    def check(entry, code, message=None, **changed):
        args = dict(defaults, **changed)
        rc = getattr(lib.c, "bitnet_hip_" + entry)(*(args[name] for name in ORDER[entry]))
        assert rc == code, (entry, changed, rc, lib.last_error())
        if code != OK:
            assert lib.last_error() == message.format(e=entry), (entry, changed)

    return check


def too_large(entry, n_layers=3, n_kv=2, max_pos=640, positions=10):
    tail = f", snapshot of {positions}" if entry in ("kv_save_dev", "kv_restore_dev") else ""
    return f"dimensions too large for this library ({{e}}: n_layers {n_layers}, n_kv_heads {n_kv}, max_pos {max_pos}{tail})"


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(refuse, entry):
    for name in ORDER[entry]:
        if name in POINTERS:
            refuse(entry, INVALID, "Null pointer passed to {e}", **{name: None})
    if entry == "kv_permute_dev":  # every argument good but the state
        refuse(entry, INVALID, "Null beam passed to {e}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_model_shape(refuse, entry):
    refuse(entry, INVALID, "{e}: n_layers 0", n_layers=0)
    refuse(entry, INVALID, "{e}: head_dim 0 unsupported (128)", head_dim=0)
    refuse(entry, INVALID, "{e}: head_dim 64 unsupported (128)", head_dim=64)
    refuse(entry, INVALID, "{e}: head_dim 256 unsupported (128)", head_dim=256)
    refuse(entry, INVALID, "{e}: num_key_value_heads 0", n_kv=0)
    refuse(entry, INVALID, "{e}: flags 0x1 (0 or BITNET_HIP_ATTN_KV_F16)", flags=1)
    refuse(entry, INVALID, "{e}: flags 0x4 (0 or BITNET_HIP_ATTN_KV_F16)", flags=4)
    refuse(entry, INVALID, "{e}: flags 0x3 (0 or BITNET_HIP_ATTN_KV_F16)", flags=KV_F16 | 1)
    refuse(entry, INVALID, "{e}: flags 0xffffffff (0 or BITNET_HIP_ATTN_KV_F16)", flags=-1)


@pytest.mark.parametrize("entry", sorted(COUNTED))
def test_destination_count(refuse, entry):
    refuse(entry, INVALID, "{e}: " + COUNTED[entry] + " 0 must be 1..8", count=0)
    refuse(entry, INVALID, "{e}: " + COUNTED[entry] + " 9 must be 1..8", count=9)


@pytest.mark.parametrize("entry", ENTRIES)
def test_position_bound(refuse, entry):
    refuse(entry, INVALID, "KV cache overflow: " + BOUND[entry] + " 641, max_pos 640", n=641, S=641)
    refuse(entry, INVALID, "KV cache overflow: " + BOUND[entry] + " 1, max_pos 0", max_pos=0, n=1, keep=0, discard=1, flags=KV_F16)


@pytest.mark.parametrize("entry", ENTRIES)
def test_sizes_that_wrap(refuse, entry):
    """the four tuples of test_kv_fork_abi.py: products that wrap size_t or pass the grid's range are refused, not multiplied"""
    refuse(entry, INVALID, too_large(entry, max_pos=BIG), max_pos=BIG)
    refuse(entry, INVALID, too_large(entry, n_kv=1 << 60, max_pos=1 << 20), n_kv=1 << 60, max_pos=1 << 20)
    refuse(entry, INVALID, too_large(entry, n_layers=1 << 40, n_kv=1 << 40), n_layers=1 << 40, n_kv=1 << 40)
    refuse(entry, INVALID, too_large(entry, n_layers=1 << 30), n_layers=1 << 30)


def test_each_entrys_own_edge(refuse):
    # shift holds positions in 32-bit ints: max_pos 2^31 - 1 is the last it takes (keep + discard == n_positions: valid, nothing to launch)
    refuse("kv_shift_dev", INVALID, too_large("kv_shift_dev", max_pos=1 << 31), max_pos=1 << 31)
    refuse("kv_shift_dev", OK, max_pos=(1 << 31) - 1, keep=5, discard=5)
    # permute rounds max_pos up to whole chunks in an int: 2^31 - 64 is the last it takes (and then asks for the state)
    refuse("kv_permute_dev", INVALID, too_large("kv_permute_dev", max_pos=(1 << 31) - 63), max_pos=(1 << 31) - 63)
    refuse("kv_permute_dev", INVALID, "Null beam passed to {e}", max_pos=(1 << 31) - 64)
    # fork, save and restore have no such edge (no positions: valid, nothing to launch) ...
    for entry in ("kv_fork_dev", "kv_save_dev", "kv_restore_dev"):
        for max_pos in (1 << 31, (1 << 31) - 63):
            refuse(entry, OK, max_pos=max_pos, n=0)
    # ... and an empty snapshot has no size that could wrap, where fork refuses the segment count whatever n_positions is
    refuse("kv_save_dev", OK, n_layers=1 << 30, n=0)
    refuse("kv_restore_dev", OK, n_layers=1 << 30, n=0, S=0)
    refuse("kv_fork_dev", INVALID, too_large("kv_fork_dev", n_layers=1 << 30), n_layers=1 << 30, n=0)
    refuse("kv_restore_dev", OK, n_layers=1 << 62, count=8, n=0, S=0)


def test_snapshot_refusals(refuse, mem):
    refuse("kv_save_dev", INVALID, "{e}: the snapshot must be 16-byte aligned", snap=mem[1] + 4)
    refuse("kv_restore_dev", INVALID, "{e}: the snapshot must be 16-byte aligned", snap=mem[1] + 8)
    refuse("kv_restore_dev", INVALID, "{e}: n_positions 10 exceeds snapshot_positions 9", S=9)
    # the order: the cache bound, what the snapshot holds, its alignment, the sizes
    refuse("kv_restore_dev", INVALID, "KV cache overflow: n_positions 641, max_pos 640", n=641, S=9, snap=mem[1] + 4)
    refuse("kv_restore_dev", INVALID, "{e}: n_positions 10 exceeds snapshot_positions 9", S=9, snap=mem[1] + 4, n_kv=1 << 60)
    refuse("kv_save_dev", INVALID, "{e}: the snapshot must be 16-byte aligned", snap=mem[1] + 4, n_kv=1 << 60)


def test_shift_refusals(refuse):
    e = "kv_shift_dev"
    refuse(e, INVALID, "{e}: discard 0 (at least one position must go)", discard=0)
    refuse(e, INVALID, "{e}: keep 6 + discard 5 exceeds n_positions 10", keep=6, discard=5)
    refuse(e, INVALID, "{e}: keep 18446744073709551615 + discard 1 exceeds n_positions 10", keep=BIG, discard=1)
    # the order: flags, discard 0, the cache bound, keep + discard, the sizes
    refuse(e, INVALID, "{e}: flags 0x1 (0 or BITNET_HIP_ATTN_KV_F16)", flags=1, discard=0)
    refuse(e, INVALID, "{e}: discard 0 (at least one position must go)", discard=0, n=641)
    refuse(e, INVALID, "KV cache overflow: n_positions 641, max_pos 640", n=641, keep=640, discard=2)
    refuse(e, INVALID, "{e}: keep 6 + discard 5 exceeds n_positions 10", keep=6, discard=5, max_pos=1 << 31)


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_faults_at_once_fix_the_order(refuse, entry):
    refuse(entry, INVALID, "{e}: n_layers 0", n_layers=0, head_dim=64)
    refuse(entry, INVALID, "{e}: flags 0x4 (0 or BITNET_HIP_ATTN_KV_F16)", flags=4, n=641, S=641)
    refuse(entry, INVALID, "KV cache overflow: " + BOUND[entry] + " 641, max_pos 640", n=641, S=641, n_kv=1 << 60)
    # shift alone names a zero num_key_value_heads before a bad head_dim
    first = "{e}: num_key_value_heads 0" if entry == "kv_shift_dev" else "{e}: head_dim 64 unsupported (128)"
    refuse(entry, INVALID, first, n_kv=0, head_dim=64)
    refuse(entry, INVALID, "{e}: head_dim 64 unsupported (128)", head_dim=64, flags=1)
    if entry in COUNTED:
        # restore counts its destinations before it looks at the model; fork and permute after n_layers
        first = "{e}: n_dst 0 must be 1..8" if entry == "kv_restore_dev" else "{e}: n_layers 0"
        refuse(entry, INVALID, first, n_layers=0, count=0)
        refuse(entry, INVALID, "{e}: " + COUNTED[entry] + " 9 must be 1..8", count=9, head_dim=64)
        refuse(entry, INVALID, "Null pointer passed to {e}", count=9, **{ORDER[entry][0]: None})


def test_permute_shows_the_geometry_before_the_state(refuse):
    refuse("kv_permute_dev", INVALID, "{e}: head_dim 64 unsupported (128)", beam=None, head_dim=64)
    refuse("kv_permute_dev", INVALID, too_large("kv_permute_dev", n_layers=1 << 30), beam=None, n_layers=1 << 30)
    refuse("kv_permute_dev", INVALID, "Null pointer passed to {e}", beam=None, k=None, head_dim=64)
