"""bzamd_inner_product_verify_batch_workspace_bytes (include/blitzar_amd.h): the size of the batch
verifier's workspace is a function of np = 2^ceil_log2(n) and num_proofs, needs no backend, and is
0 outside the limits of bzamd_verify_inner_product_batch_device."""
from blitzar_amd import api
from tests.test_inner_product_device import padded, rounds_of

SIZES = (1, 2, 3, 5, 513, 1024, 1025, 1 << 16)


def test_batch_workspace_bytes_outside_the_limits():
    size = api.inner_product_verify_batch_workspace_bytes
    assert size(0, 1) == 0
    assert size((1 << 30) + 1, 1) == 0
    assert size(1024, 0) == 0
    assert size(1024, (1 << 18) + 1) == 0  # num_proofs x np > 2^28
    assert size(1025, 1 << 18) == 0        # np = 2048
    assert size(1, (1 << 28) + 1) == 0
    assert size(1 << 28, 2) == 0
    assert size((1 << 28) + 1, 1) == 0  # np = 2^29
    assert size(1 << 28, 1) > 0
    assert size(1024, 1 << 18) > 0
    assert size(1, 1 << 28) > 0


def test_batch_workspace_bytes_depend_on_np_alone():
    size = api.inner_product_verify_batch_workspace_bytes
    for num_proofs in (1, 7, 64):
        assert size(513, num_proofs) == size(1000, num_proofs) == size(1024, num_proofs)
        assert size(1025, num_proofs) > size(1024, num_proofs) > size(512, num_proofs)


def test_batch_workspace_bytes_grow_with_num_proofs():
    size = api.inner_product_verify_batch_workspace_bytes
    for n in SIZES:
        sizes = [size(n, num_proofs) for num_proofs in range(1, 70)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), n


def test_batch_workspace_bytes_hold_the_chain():
    """per proof a shared column of np + 1 rows, an own column of 1 + 2 rounds rows and as many
    points; the np + 1 generators once"""
    size = api.inner_product_verify_batch_workspace_bytes
    for n in SIZES:
        np_, rounds = padded(n), rounds_of(n)
        own = 1 + 2 * rounds
        for num_proofs in (1, 2, 65, 256):
            assert size(n, num_proofs) >= (num_proofs * (32 * (np_ + 1) + 32 * own + 160 * own)
                                           + 160 * (np_ + 1))


def test_batch_holds_the_generators_once():
    assert (api.inner_product_verify_batch_workspace_bytes(1024, 64)
            < 64 * api.inner_product_verify_workspace_bytes(1024))


def test_batch_of_one_fits_the_single_form_workspace():
    """bzamd_verify_inner_product_device runs the batch of one in the workspace it has always
    asked for"""
    for rounds in range(0, 29):
        n = 1 << rounds
        assert (0 < api.inner_product_verify_batch_workspace_bytes(n, 1)
                <= api.inner_product_verify_workspace_bytes(n)), n
