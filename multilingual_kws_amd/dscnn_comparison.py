"""The reference's DS-CNN comparison (notebooks/dscnn_comparison.py, dscnn_comparison_filtering.py) on the device: model_def builds
the network, train is the notebook's train() (:147-195: the AudioDataset with silence, unknown and SpecAugment, the step schedule, the
best-epoch checkpoint) on the device tape of dscnn_trainer, evaluate scores a network on files with the accuracy
and confusion matrix of the notebook (:398).  A network trained elsewhere comes in through dscnn.DSCNN.from_keras / DSCNN.load."""
import os

import numpy as np

from . import dscnn, dscnn_trainer
from .embedding import input_data, transfer_learning


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


def step_function_wrapper(batch_size):
    """The reference's learning-rate schedule (:124-134); batch_size is unused there too."""
    def step_function(epoch, lr):
        if epoch < 12:
            return 0.0005
        elif epoch < 24:
            return 0.0001
        elif epoch < 36:
            return 0.00002
        else:
            return 0.00001
    return step_function


def train(commands, train_files, val_files, unknown_files, model_settings, dataset, bg_datadir, epochs=48, batch_size=100, checkpoint_dir=None, seed=10,
          verbose=1, mode=None):
    """The reference's train(): a DS-CNN of model_settings['label_count'] labels with Keras' initialisation, trained for `epochs` passes
    over train_files (label = parent directory; silence and unknown mixed in, SpecAugment on 80 % of the clips) in shuffled batches of
    batch_size, the short last batch included, under step_function_wrapper's schedule.  Every epoch the network is scored on val_files
    (with silence and unknown) through a DSCNN built from the trainer's parameters; the best epoch by validation accuracy is saved with
    dscnn.save to <checkpoint_dir>/dscnn_<dataset>.  Returns the last epoch's DSCNN with a `history` dict attached: loss (regularisation
    included, as Keras reports it), sparse_categorical_accuracy, val_loss, val_sparse_categorical_accuracy, lr.
    Augmentation draws have distribution parity with the reference, not the same values.  mode: "eager" (default) or "hipgraph"."""
    import torch
    if not os.path.isdir(bg_datadir):
        raise ValueError("no bg data at", bg_datadir)
    label_count = int(model_settings["label_count"])
    a = input_data.AudioDataset(model_settings, commands, bg_datadir, unknown_files, silence_percentage=100.0 / 6.0, unknown_percentage=100.0 / 7.0,
                                spec_aug_params=input_data.SpecAugParams(percentage=80), seed=seed)
    train_ds = a.init_from_parent_dir(None, train_files, is_training=True).shuffle(buffer_size=len(train_files)).batch(batch_size)
    val_ds = a.eval_with_silence_unknown(None, val_files, label_from_parent_dir=True).batch(batch_size)
    trainer = dscnn_trainer.DSCNNTrainer(dscnn.glorot_params(label_count, seed), label_count, max_batch=batch_size, seed=seed, mode=mode or "eager")
    schedule = step_function_wrapper(batch_size)
    history = {k: [] for k in ("loss", "sparse_categorical_accuracy", "val_loss", "val_sparse_categorical_accuracy", "lr")}
    best, model, lr = -1.0, None, 0.0001
    for epoch in range(int(epochs)):
        lr = schedule(epoch, lr)
        totals, seen, reg = torch.zeros(2, dtype=torch.float64, device=trainer.device), 0, 0.0
        for spec, labels in train_ds:
            # Keras reports the batch's loss with the L2 term of the weights the batch was run with
            reg += trainer.regularization_loss() * int(spec.shape[0])
            totals += trainer.step(spec, labels, lr).double()
            seen += int(spec.shape[0])
        loss_sum, correct = totals.cpu().tolist()
        if model is not None:
            model.close()
        model = dscnn.DSCNN(trainer.params(), label_count, max_batch=batch_size, device=trainer.device)
        vloss, vcorrect, vseen = 0.0, 0, 0
        for spec, labels in val_ds:
            probs = model.forward(spec).double()
            picked = probs.gather(1, labels.to(torch.int64).view(-1, 1)).clamp(1e-7, 1 - 1e-7)       # Keras' loss on probabilities clips them
            vloss += float(-picked.log().sum().cpu())
            vcorrect += int((probs.argmax(dim=1) == labels.to(torch.int64)).sum().cpu())
            vseen += int(spec.shape[0])
        reg_now = trainer.regularization_loss()
        history["loss"].append((loss_sum + reg) / max(seen, 1))
        history["sparse_categorical_accuracy"].append(correct / max(seen, 1))
        history["val_loss"].append(vloss / max(vseen, 1) + reg_now)
        history["val_sparse_categorical_accuracy"].append(vcorrect / max(vseen, 1))
        history["lr"].append(lr)
        if verbose:
            print(f"Epoch {epoch + 1}/{epochs} - lr {lr:g} - " + " - ".join(f"{k}: {history[k][-1]:.4f}" for k in list(history)[:4]))
        if checkpoint_dir is not None and history["val_sparse_categorical_accuracy"][-1] > best:
            best = history["val_sparse_categorical_accuracy"][-1]
            dscnn.save(os.path.join(checkpoint_dir, "dscnn_" + dataset), model.params)
    model.history = history
    return model
