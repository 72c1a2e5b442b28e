"""``MetricBase``: what the three metric loggers share -- the recorded ``metric_data``, its summaries, and the one
device-to-host copy of an ``add_sample``."""
import numpy as np
import torch

__all__ = ["MetricBase"]

BACKENDS = ("hip", "torch")


def host_copy(packed: torch.Tensor) -> np.ndarray:
    """THE device-to-host copy of an ``add_sample`` (and its only synchronisation): everything a sample records travels in
    one tensor."""
    return packed.detach().cpu().numpy()


def pack_rows(rows):
    """1-D device tensors of equal length, possibly of different dtypes -> one 2-D tensor in their common dtype (at least
    float32: numpy holds no bfloat16) and the numpy dtype each row goes back to on the host."""
    common = torch.float32
    for r in rows:
        common = torch.promote_types(common, r.dtype)
    back = [np.float64 if r.dtype == torch.float64 else np.float32 for r in rows]
    return torch.stack([r.to(common) for r in rows]), back


def unpack_rows(host, back):
    return [np.ascontiguousarray(row.astype(dt)) for row, dt in zip(host, back)]


def fusable(*tensors):
    """What the fused ops take: float32 tensors on one GPU (int64 labels are checked by the caller)."""
    first = tensors[0]
    return first.is_cuda and all(t.dtype == torch.float32 and t.device == first.device for t in tensors)


class MetricBase:
    """Records per-image metrics of every batch in ``metric_data`` (a list of one array per ``add_sample`` under each
    ``Batch_*`` key) and summarises them, as the reference's ``MetricBase``.

    ``main_metric`` may be given with or without its ``Batch_`` prefix; ``mode`` is 'training' or 'validation'.

    Out of scope here: the reference stores epochs in HDF5 files (``save_epoch``, ``load_statistics``, ``max_accuracy`` and the
    plotting methods).  ``h5py`` is not a dependency of this package, so these do not exist; ``savefile`` and ``base_dir`` are
    accepted, so that the reference's constructor calls work, and ignored: no file is touched.

    ``backend='hip'`` (default) takes the fused HIP ops for float32 CUDA tensors; ``'torch'``, and every other dtype or device,
    takes stock ops in the reference's operation order.  Either way an ``add_sample`` makes exactly one device-to-host copy.
    """

    def __init__(self, savefile, base_dir, main_metric, mode="training", backend="hip"):
        if mode not in ("training", "validation"):
            raise AssertionError("invalid mode: %s" % mode)
        if backend not in BACKENDS:
            raise ValueError("backend must be one of %s, got %r" % (BACKENDS, backend))
        self.mode = mode
        self.backend = backend
        self.metric_data = {}
        self.main_metric = main_metric if main_metric.startswith("Batch_") else "Batch_" + main_metric
        self._path = None          # no file, whatever savefile / base_dir say

    @staticmethod
    def _flat(data):
        return np.concatenate(data) if isinstance(data[0], np.ndarray) else np.asarray(data).ravel()

    def get_current_statistics(self, main_only=True, return_loss=True):
        """(means, sample variances) of the recorded epoch: of the main metric, then the loss, or with ``main_only=False`` of
        every ``Batch_*`` key in sorted order."""
        means, variances = (), ()
        if main_only:
            keys = [self.main_metric] + (["Batch_Loss"] if return_loss else [])
        else:
            keys = [k for k in sorted(self.metric_data) if k.startswith("Batch") and (return_loss or k != "Batch_Loss")]
        for key in keys:
            data = self._flat(self.metric_data[key])
            means += (data.mean(),)
            variances += (data.var(ddof=1),)
        return means, variances

    def get_last_batch(self, main_metric=True):
        """The last batch's main metric (mean over its images, NaN entries left out), or every metric's last array."""
        if main_metric:
            return np.nanmean(self.metric_data[self.main_metric][-1])
        return tuple(self.metric_data[k][-1] for k in sorted(self.metric_data) if k != "Batch_Loss")

    def print_epoch_statistics(self):
        for key, data in self.metric_data.items():
            print("%s: %.3f" % (key.replace("Batch_", ""), np.asarray(data).mean()))

    @staticmethod
    def _confmat_cls_pr_rc(conf_mat: np.ndarray):
        """Class-wise (precision, recall) of a confusion matrix [label, prediction]: the diagonal over the column sums and
        over the row sums."""
        hits = np.diag(conf_mat)
        return hits / np.sum(conf_mat, axis=0), hits / np.sum(conf_mat, axis=1)

    def _reset_metric(self):
        raise NotImplementedError

    def add_sample(self, predictions, targets, loss=0, **kwargs):
        raise NotImplementedError
