"""The reference's DS-CNN comparison (notebooks/dscnn_comparison.py, dscnn_comparison_filtering.py) on the device: model_def builds
the network, evaluate scores it on files with the accuracy and confusion matrix of the notebook (:398).  Inference only -- a trained
network comes in through dscnn.DSCNN.from_keras / DSCNN.load; training it is not built."""
import numpy as np

from . import dscnn
from .embedding import transfer_learning


def model_def(label_count, seed=None, max_batch=1024, device=None):
    """A DSCNN with Keras' default initialisation (Glorot-uniform kernels, zero biases, BatchNorm ones and zeros): what the reference's
    model_def(label_count) returns before it is trained."""
    return dscnn.DSCNN(dscnn.glorot_params(label_count, seed), label_count, max_batch=max_batch, device=device)


def evaluate(model, files, labels, model_settings, convert=False):
    """Classifies `files` (true classes `labels`) -> dict(accuracy, confusion_matrix [L,L] int64 with rows = true class, predictions).
    The files go through the same reader and frontend as the few-shot models'; the confusion matrix is counted on the device."""
    import torch
    L = model.label_count
    labels = np.asarray(labels, dtype=np.int64)
    if labels.shape != (len(files),) or (labels.size and (labels.min() < 0 or labels.max() >= L)):
        raise ValueError(f"labels must be {len(files)} classes in [0, {L})")
    specs = transfer_learning._specs_for_files(list(files), model_settings, convert=convert)
    d_specs = torch.from_numpy(np.ascontiguousarray(specs, dtype=np.float32)).to(model.device)
    pred = [model.forward(d_specs[s:s + model.max_batch]).argmax(dim=1) for s in range(0, len(files), model.max_batch)]
    pred = torch.cat(pred) if pred else torch.zeros(0, dtype=torch.int64, device=model.device)
    true = torch.from_numpy(labels).to(model.device)
    confusion = torch.bincount(true * L + pred, minlength=L * L).view(L, L)
    accuracy = float((pred == true).double().mean().cpu()) if len(files) else float("nan")
    return dict(accuracy=accuracy, confusion_matrix=confusion.cpu().numpy().astype(np.int64), predictions=pred.cpu().numpy())
