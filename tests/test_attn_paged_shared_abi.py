"""CPU: the C ABI of the fork groups' paged decode attention (include/bitnet_hip_pagedshared.h): every refusal comes back as INVALID_ARGUMENT before
anything launches (the pointers here are never dereferenced), the scratch size is monotone and 0 for refused geometry, the names are exported."""
import pytest

H, N_KV, D, MAX_POS, N_PAGES, P = 8, 2, 128, 576, 32, 0x1000  # P: a non-null pointer no refusal path reads


def call(hip, n_seq=4, leader=(0, 0, 2, 3), shared=(2, 2, 0, 0), nss=0, n_pages=N_PAGES, key_bound=MAX_POS, n_splits=1, head_dim=D):
    hip.attention_decode_paged_shared_dev(P, P, P, P, P, n_pages, P, P, n_seq, H, N_KV, head_dim, MAX_POS, key_bound, n_splits, P, P, leader, shared, nss)


@pytest.mark.parametrize("kw", (
    dict(n_seq=65), dict(head_dim=64), dict(n_pages=0), dict(key_bound=MAX_POS + 1), dict(n_splits=10),  # the paged entry's own
    dict(leader=None), dict(shared=None),
    dict(leader=(0, 4, 2, 3)), dict(leader=(0, -1, 2, 3)),      # outside [0, n_seq)
    dict(leader=(0, 2, 3, 3)),                                   # leader[leader[1]] != leader[1]
    dict(shared=(2, 1, 0, 0)), dict(shared=(2, 2, -1, 0)),       # differing inside a group, negative
    dict(shared=(9, 9, 0, 0)), dict(shared=(1, 1, 0, 0), key_bound=64),  # above ceil(key_bound / 64) - 1
    dict(nss=3), dict(shared=(0, 0, 0, 0), nss=1),               # above the largest S
), ids=str)
def test_refusals_come_before_any_launch(pkg, kw):
    with pytest.raises(pkg.BitNetHipError) as e:
        call(pkg.load(), **kw)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT


def test_scratch_bytes_and_names(pkg):
    hip = pkg.load()
    rec = (8 + 4 * D) * 4
    base = hip.attention_paged_scratch_bytes(5, N_KV, 3)
    sizes = [hip.attention_paged_shared_scratch_bytes(5, N_KV, 3, s) for s in range(5)]
    assert sizes == [base + 5 * N_KV * s * rec for s in range(5)]
    assert hip.attention_paged_shared_scratch_bytes(6, N_KV, 3, 2) > sizes[2] < hip.attention_paged_shared_scratch_bytes(5, N_KV, 4, 2)
    assert [hip.attention_paged_shared_scratch_bytes(*g) for g in ((0, 2, 1, 1), (65, 2, 1, 1), (4, 0, 1, 1), (4, 2, 0, 1), (4, 2, 1, 2 ** 62))] == [0] * 5
    # the library's shared split rule: min(S, 16, ceil(512 / (groups * kv)))
    assert [hip.attention_paged_shared_splits(*g) for g in ((1, 5, 64), (1, 5, 3), (8, 20, 64), (0, 5, 64), (1, 5, 0))] == [16, 3, 4, 0, 0]
    names = {n for n, _, _ in pkg.pagedshared_prototypes()}
    assert names == {"bitnet_hip_attention_paged_shared_splits", "bitnet_hip_attention_paged_shared_scratch_bytes", "bitnet_hip_attention_decode_paged_shared_dev"}
    assert names <= set(pkg.declared_symbols()) and all(hasattr(hip.c, n) for n in names)
