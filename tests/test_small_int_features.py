"""The batch property "every atom-feature element is an integer with |x| <= 256 / max_deg" (include/gcmi.h:
gcmi_model_io.features_small_int), as the host collation establishes it while it copies the rows.  No GPU: integer
and comparison work, every answer is exact."""
import numpy as np
import pytest

from deepchem_amd.data.collate import collate_host
from deepchem_amd.feat.atom_codes import features_from_codes
from deepchem_amd.utils.synthetic import PackedMols, synthetic_molecules

LIMIT = 25  # 256 // max_deg for the model's max_deg of 10


def _small_int(features, limit=LIMIT):
    """The definition, in numpy."""
    f = np.asarray(features, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(f) & (np.abs(f) <= limit) & (f == np.trunc(f))))


def _with(packed, row, col, value):
    f = np.array(packed.atom_features, np.float32, copy=True)
    f[row, col] = value
    return PackedMols(f, packed.atom_ptr, packed.adj_ptr, packed.adj_idx)


def test_zero_one_rows_have_the_property():
    packed = synthetic_molecules(300, seed=4)
    assert _small_int(packed.atom_features)
    hb = collate_host(packed, None, pin=False)
    assert hb.small_int and hb.symmetric


@pytest.mark.parametrize("value,expected", [(25.0, True), (26.0, False), (0.5, False), (-3.0, True), (-25.0, True),
                                            (-26.0, False), (float("nan"), False), (float("inf"), False),
                                            (float("-inf"), False), (-0.0, True), (1e-30, False), (3e9, False)])
def test_one_element_decides(value, expected):
    packed = synthetic_molecules(120, seed=7)
    n_atoms, n_feat = packed.atom_features.shape
    for row, col in ((0, 0), (n_atoms // 2, 31), (n_atoms - 1, n_feat - 1)):  # first, middle and last element
        p = _with(packed, row, col, value)
        assert _small_int(p.atom_features) == expected
        hb = collate_host(p, None, pin=False)
        assert hb.small_int == expected, (value, row, col)
        assert hb.symmetric  # the adjacency's property does not depend on the features


def test_limit_follows_max_deg():
    """|x| <= 256 // max_deg: a sum over max_deg neighbours stays below 256 (exact in bf16)."""
    packed = synthetic_molecules(60, seed=2, max_atoms=12)
    deg = int(np.diff(packed.adj_ptr).max())
    assert deg <= 6
    for max_deg, ok, bad in ((10, 25, 26), (6, 42, 43)):
        assert collate_host(_with(packed, 5, 5, ok), None, max_deg=max_deg, pin=False).small_int
        assert not collate_host(_with(packed, 5, 5, bad), None, max_deg=max_deg, pin=False).small_int


def test_selection_decides_not_the_set():
    """The property belongs to the batch: a set with one offending molecule gives clean batches without it."""
    packed = synthetic_molecules(50, seed=9)
    bad_mol = 17
    p = _with(packed, int(packed.atom_ptr[bad_mol]), 3, 0.25)
    sel_without = np.array([m for m in range(50) if m != bad_mol], np.int64)
    assert collate_host(p, sel_without, pin=False).small_int
    assert not collate_host(p, np.array([3, bad_mol, 5], np.int64), pin=False).small_int
    assert not collate_host(p, None, pin=False).small_int


def test_answer_does_not_depend_on_the_thread_count():
    """One worker per 256 molecules (up to 16): 100 molecules are collated by one thread, 4 000 by fifteen.  The
    violation sits in the first, a middle and the last molecule in turn, so every worker position is exercised."""
    small = synthetic_molecules(100, seed=1, max_atoms=12)
    large = synthetic_molecules(4000, seed=1, max_atoms=12)
    for packed in (small, large):
        assert collate_host(packed, None, pin=False).small_int
        for mol in (0, packed.n_mols // 2, packed.n_mols - 1):
            p = _with(packed, int(packed.atom_ptr[mol]), 11, 7.5)
            hb = collate_host(p, None, pin=False)
            assert not hb.small_int and hb.symmetric


def _coded_single_atoms(codes):
    n = codes.shape[0]
    atom_ptr = np.arange(n + 1, dtype=np.int64)
    adj_ptr = np.zeros(n + 1, np.int64)
    return PackedMols(None, atom_ptr, adj_ptr, np.zeros(0, np.int32), atom_codes=codes)


def test_every_atom_code_value():
    """Atom codes expand to one-hot blocks (0 / 1) and three VALUES: formal charge (int8), radical electrons and the
    aromatic byte.  So a coded batch has the property exactly when those three bytes are within the limit -- checked
    here for every value of every code byte against the definition applied to the expanded row."""
    for byte in range(8):
        codes = np.zeros((256, 8), np.uint8)
        codes[:, byte] = np.arange(256, dtype=np.uint8)
        rows = features_from_codes(codes)
        for v in range(256):
            expected = _small_int(rows[v])
            hb = collate_host(_coded_single_atoms(codes[v:v + 1]), None, pin=False)
            assert hb.small_int == expected, (byte, v)
            if byte in (0, 1, 2, 5, 7):  # one-hot bytes: any value expands to a 0 / 1 row
                assert expected
    # ... and a batch of featurizer-shaped codes (charges -2..2, 0..2 radicals, aromatic 0 / 1) has it
    rng = np.random.RandomState(3)
    codes = np.zeros((500, 8), np.uint8)
    codes[:, 0] = rng.randint(0, 44, 500)
    codes[:, 1] = rng.randint(0, 11, 500)
    codes[:, 3] = rng.randint(-2, 3, 500).astype(np.int8).view(np.uint8)
    codes[:, 4] = rng.randint(0, 3, 500)
    codes[:, 6] = rng.randint(0, 2, 500)
    assert _small_int(features_from_codes(codes))
    assert collate_host(_coded_single_atoms(codes), None, pin=False).small_int


def test_hand_built_batches_make_no_promise():
    """DeviceBatch(...) from a tensor, BatchGraph(...) by hand: false unless stated."""
    import inspect
    from deepchem_amd.data.collate import DeviceBatch
    assert inspect.signature(DeviceBatch.__init__).parameters["small_int_features"].default is False
