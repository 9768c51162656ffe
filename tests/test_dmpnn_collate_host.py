"""gcmi_dmpnn_collate_host: the index routine of the device collation (the same __host__ __device__ code as the kernel
of gcmi_dmpnn_collate) run by host loops.  Its buffer must be, word for word, what DmpnnBatch.to() packs from the
numpy-collated batch -- no arithmetic is involved, so the comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

from deepchem_amd import _lib, ops
from deepchem_amd.models.torch_models.dmpnn import (DmpnnBatch, DmpnnGraphSet, ResidentDmpnnSet, pack_batch_words,
                                                   split_batch_words)
from tests import dmpnn_collate_cases as C
from tests import dmpnn_refs as R


def test_a_single_atom_without_bonds_is_an_empty_run():
    gs = C.graph_set(5, 2, 0)
    for m in (C.LONE_FIRST, C.LONE_LAST):
        assert gs.atom_ptr[m + 1] - gs.atom_ptr[m] == 1 and gs.bond_ptr[m + 1] == gs.bond_ptr[m]
    host = gs.batch([C.LONE_LAST]).host
    assert host["out_ptr"].tolist() == [0, 0] and host["rev"].size == 0 and host["f_ini_atoms_bonds"].shape == (0, 7)
    rs = C.resident_host(5, 2, 0)
    assert rs.host_arrays["out_start"][0] == 0 and rs.host_arrays["out_start"][-1] == 0


def test_out_start_is_the_prefix_of_the_out_degrees_inside_the_molecule():
    gs, rs = C.graph_set(5, 2, 4), C.resident_host(5, 2, 4)
    for m in range(gs.n_mols):
        a0, a1 = gs.atom_ptr[m], gs.atom_ptr[m + 1]
        want = np.concatenate([[0], np.cumsum(gs.out_degree[a0:a1])[:-1]]) if a1 > a0 else np.zeros(0)
        assert np.array_equal(rs.host_arrays["out_start"][a0:a1], want), m
    assert np.array_equal(rs.host_arrays["bond_features"], gs.bond_features[gs.order])


@pytest.mark.parametrize("name", sorted(C.SELECTIONS))
@pytest.mark.parametrize("widths", C.WIDTHS, ids=lambda w: "%dx%dx%d" % w)
def test_host_routine_writes_the_words_to_packs(widths, name):
    rs = C.resident_host(*widths)
    batch, want, layout = C.reference(widths, name)
    plan, n_atoms, n_bonds = rs.plan(C.SELECTIONS[name])
    assert (n_atoms, n_bonds) == (batch.n_atoms, batch.n_bonds)
    out = np.frombuffer(b"\xff" * (4 * want.size), np.int32).copy()  # an unwritten word, pad words included, shows
    got = ops.dmpnn_collate_host(rs.host_arrays, plan.numpy(), len(C.SELECTIONS[name]), n_atoms, n_bonds, out=out)
    assert got is out
    assert np.array_equal(got, want)
    blocks = split_batch_words(got, layout)
    assert list(blocks) == list(batch.host) == list(ops.DMPNN_BATCH_BLOCKS)
    for k, a in batch.host.items():
        assert blocks[k].dtype == a.dtype and blocks[k].shape == a.shape and np.array_equal(blocks[k], a), k
        assert layout[k][0] % 4 == 0, k


def test_pad_words_exist_in_the_pads_case():
    _, words, layout = C.reference((133, 14, 0), "pads")
    sizes = {k: int(np.prod(shape)) for k, (_, shape) in layout.items()}
    assert sum(1 for k in sizes if sizes[k] % 4) >= 4
    assert words.size == sum((n + 3) // 4 * 4 for n in sizes.values())


def test_a_longer_output_buffer_is_left_alone_past_the_layout():
    widths = (8, 4, 4)
    rs = C.resident_host(*widths)
    _, want, _ = C.reference(widths, "repeats")
    plan, n_atoms, n_bonds = rs.plan(C.SELECTIONS["repeats"])
    out = np.full(want.size + 5, -1, np.int32)
    ops.dmpnn_collate_host(rs.host_arrays, plan.numpy(), 5, n_atoms, n_bonds, out=out)
    assert np.array_equal(out[:want.size], want) and np.all(out[want.size:] == -1)


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib.load()
    rs = C.resident_host(5, 2, 4)
    sel = C.SELECTIONS["repeats"]
    plan, n_atoms, n_bonds = rs.plan(sel)
    words, _ = ops.dmpnn_batch_layout(len(sel), n_atoms, n_bonds, 5, 2, 4)
    out = np.full(words, -1, np.int32)
    ptr = {k: a.ctypes.data for k, a in rs.host_arrays.items()}

    def call(n_mols=len(sel), n_atoms=n_atoms, n_bonds=n_bonds, out_ptr=out.ctypes.data, out_words=words, fa=5,
             plan_ptr=plan.numpy().ctypes.data, **nulls):
        args = [None if k in nulls else ptr[k] for k in ops.DMPNN_SET_ARRAYS]
        return lib.gcmi_dmpnn_collate_host(*args, rs.graphs.n_mols, fa, 2, 4, plan_ptr, n_mols, n_atoms, n_bonds,
                                           out_ptr, out_words)

    assert call(out_words=words - 1) == -1 and b"output buffer" in lib.gcmi_last_error()
    assert call(out_ptr=None) == -1 and b"NULL" in lib.gcmi_last_error()
    assert call(plan_ptr=None) == -1 and b"NULL" in lib.gcmi_last_error()
    for k in ops.DMPNN_SET_ARRAYS:
        assert call(**{k: True}) == -1 and b"NULL" in lib.gcmi_last_error(), k
    for bad in (dict(n_mols=-1), dict(n_atoms=-1), dict(n_bonds=-1), dict(fa=-1)):
        assert call(**bad) == -1 and b"negative" in lib.gcmi_last_error(), bad
    assert np.all(out == -1)  # nothing was written by a refused call
    assert call() == 0
    # the device entry makes the same checks before any launch (no pointer is followed here)
    args = [ptr[k] for k in ops.DMPNN_SET_ARRAYS]
    tail = (rs.graphs.n_mols, 5, 2, 4, plan.numpy().ctypes.data, len(sel), n_atoms, n_bonds)
    assert lib.gcmi_dmpnn_collate(*args, *tail, out.ctypes.data, words - 1, None) == -1
    assert b"output buffer" in lib.gcmi_last_error()
    assert lib.gcmi_dmpnn_collate(*args, *tail, None, words, None) == -1 and b"NULL" in lib.gcmi_last_error()
    assert lib.gcmi_dmpnn_collate(*args[:-1], None, *tail, out.ctypes.data, words, None) == -1
    assert lib.gcmi_dmpnn_collate_words(-1, 0, 0, 5, 2, 4, None) == -1
    with pytest.raises(ValueError, match="3 \\* n_mols \\+ 2"):
        ops.dmpnn_collate_host(rs.host_arrays, plan.numpy()[:-1], len(sel), n_atoms, n_bonds)


def test_a_molecule_index_outside_the_set_is_refused_before_anything_runs():
    rs = C.resident_host(5, 2, 0)
    for bad in ([0, C.N_GRAPHS], [-1]):
        with pytest.raises(ValueError, match="outside the graph set"):
            rs.plan(bad)


def test_the_routine_skips_a_bad_entry_and_does_not_read_through_it():
    """Defence in depth under the Python check: entry 1 of the plan names molecule M + 7.  The words its molecule would
    own stay as they were, every other molecule's are written as usual."""
    widths = (5, 2, 4)
    rs = C.resident_host(*widths)
    sel = np.array([C.RING6, C.CHAIN3, C.RND_A])
    batch, want, layout = C.graph_set(*widths).batch(sel), None, None
    want, layout = pack_batch_words(batch.host)
    plan, n_atoms, n_bonds = rs.plan(sel)
    words = plan.numpy().copy()
    words[1] = C.N_GRAPHS + 7
    out = np.full(want.size, -1, np.int32)
    ops.dmpnn_collate_host(rs.host_arrays, words, 3, n_atoms, n_bonds, out=out)
    a0, a1 = batch.host["mol_ptr"][1:3]
    b0, b1 = batch.host["out_ptr"][a0], batch.host["out_ptr"][a1]
    got = split_batch_words(out, layout)
    for k in ("atom_features", "atom_membership"):
        assert np.array_equal(np.delete(got[k], np.s_[a0:a1], 0), np.delete(batch.host[k], np.s_[a0:a1], 0)), k
        assert np.all(got[k][a0:a1].view(np.int32) == -1), k
    for k in ("f_ini_atoms_bonds", "rev", "bond_src"):
        assert np.array_equal(np.delete(got[k], np.s_[b0:b1], 0), np.delete(batch.host[k], np.s_[b0:b1], 0)), k
        assert np.all(got[k][b0:b1].view(np.int32) == -1), k
    assert np.array_equal(got["mol_ptr"], batch.host["mol_ptr"])
    assert got["atoms_per_mol"].reshape(-1).tolist() == [6.0, 0.0, 9.0] and np.all(got["global_features"][1] == 0)


def test_the_resident_set_checks_the_degree_cap_once():
    rng = np.random.RandomState(0)
    graphs = [R.graph(rng, R.chain(3), 3, 5, 2, 0), R.graph(rng, R.star(33), 34, 5, 2, 0)]
    gs = DmpnnGraphSet(graphs)
    with pytest.raises(ValueError, match="an atom has 33 bonds; the D-MPNN kernels cover a degree of at most 32"):
        ResidentDmpnnSet(gs, torch.device("cpu"))
    with pytest.raises(ValueError, match="degree of at most 32"):  # the text of the per-batch check
        gs.batch([1])
    ResidentDmpnnSet(DmpnnGraphSet(graphs[:1]), torch.device("cpu"))


def test_to_and_from_device_share_the_layout_routine():
    """DmpnnBatch.to packs with pack_batch_words; a batch wrapped around the same words exposes the same attributes."""
    widths = (133, 14, 4)
    batch, words, layout = C.reference(widths, "repeats")
    moved = C.graph_set(*widths).batch(C.SELECTIONS["repeats"]).to("cpu")
    wrapped = DmpnnBatch.from_device(C.graph_set(*widths), C.SELECTIONS["repeats"], torch.from_numpy(words.copy()),
                                     batch.n_atoms, batch.n_bonds)
    assert wrapped._host is None
    for k in ops.DMPNN_BATCH_BLOCKS:
        a, b = getattr(moved, k), getattr(wrapped, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0, k
    assert (wrapped.n_mols, wrapped.n_atoms, wrapped.n_bonds) == (batch.n_mols, batch.n_atoms, batch.n_bonds)
    assert wrapped.molecules_unbatch_key == batch.molecules_unbatch_key
    for k, a in batch.host.items():
        assert np.array_equal(wrapped.host[k], a) and wrapped.host[k].dtype == a.dtype, k
    for x, y in zip(wrapped.to_reference_arrays(), batch.to_reference_arrays()):
        assert np.array_equal(x, y)
    assert wrapped.plan.n_atoms == batch.n_atoms and wrapped.plan.n_bonds == batch.n_bonds
    with pytest.raises(ValueError, match="int32 words of the layout"):
        DmpnnBatch.from_device(C.graph_set(*widths), C.SELECTIONS["repeats"], torch.from_numpy(words[:-4].copy()),
                               batch.n_atoms, batch.n_bonds)


def test_collate_argument_of_the_model():
    import deepchem_amd as dc
    with pytest.raises(ValueError, match="collate must be"):
        dc.models.DMPNNModel(collate="gpu", device=torch.device("cpu"))
