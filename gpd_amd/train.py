"""python -m gpd_amd.train TRAIN_DIR [--test TEST_DIR] [--epochs 10] [--batch 64] [--seed S] --out DIR

Trains pytorch/network.py::Net on the device as pytorch/train_net3.py does (softmax cross-entropy, Adam 1e-3 with weight decay
5e-4, batches of 64) from the train_images.npy / train_labels.npy pair that generate_data writes (TEST_DIR: the test_images.npy /
test_labels.npy pair), without a conversion to HDF5 and without torch.  Both sets are resident on the device; an epoch is one
call of gpd_hip_train_steps.  Departures from the script, both deliberate: the initial state is the seeded
gpd_hip_train_init_state, not torch's bits, and an epoch's order is gpd_hip_shuffle_orders' with the last, short batch kept
(the script's DataLoader does not shuffle).  Per epoch it prints the running loss every 1000 batches and at the end, and the
accuracy on the test set, as the script does.

DIR receives what gpd_amd.torch_export writes — the eight tensors in torch layout and network.cfg (layout = torch) — and, where
torch imports, model.pwf (torch.save of the state dict, what the script saves).
"""
import argparse
import os
import sys

import numpy as np

from gpd_amd import api, torch_export


def load_set(directory, prefix, channels=None):
    img = np.load(os.path.join(directory, prefix + "_images.npy"))
    lab = np.load(os.path.join(directory, prefix + "_labels.npy")).reshape(-1)
    if img.ndim != 4 or img.shape[1:3] != (60, 60) or img.shape[0] != len(lab):
        raise ValueError("%s: %s_images.npy %s / %s_labels.npy %s are not [n,60,60,C] / [n]" % (directory, prefix, img.shape, prefix, lab.shape))
    if channels is not None and img.shape[3] != channels:
        raise ValueError("%s: %d channels, the training set has %d" % (directory, img.shape[3], channels))
    return np.ascontiguousarray(img, np.uint8), np.ascontiguousarray(lab, np.uint8)


def train(trainer, n, epochs, batch, seed, n_test=0, log=print):
    """`epochs` passes over the trainer's resident training set of n images -> the final state."""
    for epoch, order in enumerate(api.shuffle_orders(seed, [n] * epochs)):
        full = (n // batch) * batch
        losses = trainer.steps(order[:full].reshape(-1, batch)) if full else np.zeros(0, np.float32)
        if full < n:  # the short last batch: nothing is dropped
            losses = np.concatenate([losses, trainer.steps(order[full:].reshape(1, -1))])
        for i in range(999, len(losses), 1000):
            log("[%d, %5d] loss: %.3f" % (epoch + 1, i + 1, float(losses[i - 999:i + 1].mean())))
        if len(losses) % 1000:
            log("[%d, %5d] loss: %.3f" % (epoch + 1, len(losses), float(losses[len(losses) // 1000 * 1000:].mean())))
        if n_test:
            _, correct = trainer.eval(n=n_test, which=1)
            log("epoch: %d, correct: %d, total: %d, accuracy: %.3f" % (epoch + 1, correct, n_test, correct / n_test))
    return trainer.get_state()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gpd_amd.train", description="train the grasp network on the device")
    ap.add_argument("train_dir", help="directory with train_images.npy and train_labels.npy (generate_data)")
    ap.add_argument("--test", help="directory with test_images.npy and test_labels.npy")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0, help="of the initial state and of the epochs' orders")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="parameter directory to write")
    a = ap.parse_args(argv)
    img, lab = load_set(a.train_dir, "train")
    C = img.shape[3]
    ctx = api.Context(api.default_params(C), device=a.device)
    trainer = api.Trainer(ctx, max_batch=a.batch)
    try:
        trainer.set_state(api.init_state(C, a.seed))
        trainer.set_data(img, lab, 0)
        n_test = 0
        if a.test:
            timg, tlab = load_set(a.test, "test", C)
            trainer.set_data(timg, tlab, 1)
            n_test = len(tlab)
        print("training on %d images of %d channels%s" % (len(lab), C, ", testing on %d" % n_test if n_test else ""))
        state = train(trainer, len(lab), a.epochs, a.batch, a.seed, n_test)
        names = torch_export.export(state, a.out, float(trainer.params.input_scale))
    finally:
        trainer.close()
        ctx.close()
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None:
        torch.save({k: torch.from_numpy(v.copy()) for k, v in state.items()}, os.path.join(a.out, "model.pwf"))
        names.append("model.pwf")
    print("wrote %s: %s" % (a.out, " ".join(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
