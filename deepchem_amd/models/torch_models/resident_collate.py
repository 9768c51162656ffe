"""``ResidentCollateMixin``: where ``DMPNNModel`` and ``MEGNetModel`` gather the batches of a ``NumpyDataset`` of
``GraphData``.  The flat arrays of the whole dataset are built once (the model's graph set, cached); a batch is then an
index gather over them: in numpy (``collate="host"``) or by the device over a ``data.resident.ResidentGraphSet``
(``"device"``: a ``ValueError`` naming the reason where that cannot be done) -- the same bytes either way.  ``"auto"``: the
device where ``_device_collate_refusal`` finds nothing against it and the batch size is at least the model's threshold."""
import os
from typing import Optional

import numpy as np
import torch

from deepchem_amd.data.datasets import NumpyDataset


def check_collate(collate: str) -> str:
    if collate not in ("auto", "host", "device"):
        raise ValueError("collate must be 'auto', 'host' or 'device' (got %r)" % (collate,))
    return collate


class ResidentCollateMixin(object):
    """A model sets ``self.collate = check_collate(collate)`` and states ``resident_set_class``, ``_name`` (for the
    messages), ``_device_collate_min()`` (``collate="auto"`` takes the device from that batch size up; read per call),
    ``_new_graph_set(X)`` (its graph set, after whatever it checks once per set), ``_host_batch(graphs, idx)`` and,
    where it has them, ``_set_key`` and ``_own_refusal``."""

    # (key, value) each: key = (X, *_set_key()), X compared by identity and the rest by equality
    _graph_set = None  # value: the model's graph set
    _resident = None   # value: the resident set, or the reason why there is none

    def _set_key(self) -> tuple:  # what, beyond X, a cached set depends on
        return ()

    def _own_refusal(self) -> Optional[str]:  # the model's own reason against the device collation on a GPU
        return None

    def _holds(self, held, X) -> bool:
        return held is not None and held[0][0] is X and held[0][1:] == self._set_key()

    def graph_set(self, X):
        """The flat arrays of ``X`` (an array of ``GraphData``), kept until another array (or key) is asked for."""
        if not self._holds(self._graph_set, X):
            self._graph_set = ((X,) + self._set_key(), self._new_graph_set(X))
        return self._graph_set[1]

    def _device_collate_refusal(self) -> Optional[str]:
        """What, apart from the dataset, keeps the batches from being collated on the device; None: nothing."""
        if self.device.type != "cuda":
            return "the model is on %s, not on a GPU" % self.device
        own = self._own_refusal()
        if own is not None:
            return own
        if os.environ.get("GCMI_RESIDENT_SET", "1") == "0":
            return "GCMI_RESIDENT_SET=0 switches resident sets off"
        return None

    def _resident_for(self, X):
        """The resident set of ``X``, uploaded once and kept until another array is asked for -- or, as a string, why
        there is none: the set must fit into a quarter of the device memory that is free when it is built."""
        if not self._holds(self._resident, X):
            graphs = self.graph_set(X)
            need = self.resident_set_class.bytes_needed(graphs)
            free = torch.cuda.mem_get_info(self.device)[0] if self.device.type == "cuda" else need * 4
            if need > free // 4:
                made = "the set needs %d bytes, more than a quarter of the %d free on the device" % (need, free)
            else:
                made = self.resident_set_class(graphs, self.device)
            self._resident = ((X,) + self._set_key(), made)
        return self._resident[1]

    def resident_set(self, X):
        """The graphs of ``X`` in device memory (cached); a ``ValueError`` where the set does not fit there."""
        made = self._resident_for(X)
        if isinstance(made, str):
            raise ValueError("%s: no resident graph set: %s" % (self._name, made))
        return made

    def _route(self, X):
        """The resident set that collates the batches of ``X`` on the device, or None: the host collates them."""
        if self.collate == "host":
            return None
        why = self._device_collate_refusal()
        if why is None:
            if self.collate == "auto" and self.batch_size < self._device_collate_min():
                return None  # (a preference, not an obstacle: collate="device" goes below it)
            made = self._resident_for(X)
            if not isinstance(made, str):
                return made
            why = made
        if self.collate == "device":
            raise ValueError("%s(collate='device'): %s" % (self._name, why))
        return None

    def _collated_batches(self, dataset, epochs: int, mode: str, deterministic: bool, pad_batches: bool):
        """For a ``NumpyDataset`` of graphs: the graph INDICES follow the dataset's own batch walk (same order, same
        shuffles from ``np.random``), a batch is an index gather over the cached flat arrays: by numpy (``_host_batch``)
        or, where ``_route`` says so, by the device over the resident set.  Anything else: ``default_generator``."""
        X = getattr(dataset, "X", None) if isinstance(dataset, NumpyDataset) else None
        if not (isinstance(X, np.ndarray) and X.dtype == object and X.ndim == 1):
            if self.collate == "device":
                raise ValueError("%s(collate='device'): the dataset is not a NumpyDataset of GraphData" % self._name)
            yield from self.default_generator(dataset, epochs=epochs, mode=mode, deterministic=deterministic,
                                              pad_batches=pad_batches)
            return
        graphs = self.graph_set(X)
        resident = self._route(X)
        index_set = NumpyDataset(np.arange(X.shape[0]), dataset.y, dataset.w, dataset.ids)
        for _ in range(epochs):
            for (idx, y_b, w_b, _ids) in index_set.iterbatches(batch_size=self.batch_size, deterministic=deterministic,
                                                               pad_batches=pad_batches):
                made = self._host_batch(graphs, idx) if resident is None else resident.batch(idx)
                yield (made, [y_b], [w_b])
