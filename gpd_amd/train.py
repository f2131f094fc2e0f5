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

python -m gpd_amd.train TRAIN_DIR [--test TEST_DIR] --recipe caffe [--max-iter 10000] [--snapshot N] [--resume DIR]
                        [--init DIR] [--freeze NAME[,NAME...]] [--seed S] --out DIR

trains the network the context scores by default — the reference's Caffe LeNet, no ReLU behind the convolutions — with the
reference's Caffe recipe (models/caffe/15channels/lenet_solver_15_channels.prototxt and the train_val prototxt): xavier
initialisation (the seeded gpd_hip_train_init_xavier), SGD with momentum 0.9, base_lr 0.01, weight_decay 5e-4, lr_policy inv
(gamma 1e-4, power 0.75), batches of 64 walked through shuffled passes over the set, --max-iter iterations, a test phase every
100 iterations over min(10000, n_test) test images that prints iteration, learning rate, loss and accuracy.  --snapshot N
writes OUT/snapshot_<iteration>/ (state.npz, solver.npz) every N iterations and --resume continues from such a directory, byte
for byte.  --init DIR starts from an Eigen-layout parameter directory and --freeze sets the named tensors' lr_mult to 0
(conv1.weight ... fc2.bias; a layer name such as conv1 means both of its tensors): together they fit a missing ip1 under
shipped convolutions (a file the --init DIR lacks starts from the xavier filler).  DIR receives what gpd_amd.eigen_export
writes: the eight files of the reference's EigenClassifier, ready to be a `weights_file`.

python -m gpd_amd.train --generate CONFIG [--epochs ... | --recipe caffe ...] --out DIR

takes no TRAIN_DIR: CONFIG is a generate_data configuration, and the two resident sets are filled on the device by
gpd_amd.hostlib.generate_data — every view one gpd_hip_train_append_view, every object's ranges shuffled by
gpd_hip_train_reorder — to the bytes the four .npy files would hold, which are never written; the trainer has CONFIG's
image_num_channels and runs on its hip_device.  Training then goes on exactly as above.

python -m gpd_amd.train TRAIN_DIR ... --devices 0,1,...

trains on several devices as pytorch/train_net3.py does under nn.DataParallel (:97-99), with either recipe: one replica per
listed device — a device listed twice carries two — each on a context of its own, stepped together by api.TrainerGroup
(gpd_hip_train_group_steps: every replica applies the fixed-order mean of the replicas' gradients, and no parameter leaves the
devices).  --batch stays the GLOBAL batch and must be divisible by the number of replicas G.  Replica r holds training images
r, r + G, r + 2 G, ... and walks them in its own orders, gpd_hip_shuffle_orders((seed + 1000003 (r + 1)) & 0xffffffff, ...) over
its shard; an epoch (a pass, under the Caffe recipe) is min_r(n_r) // (batch / G) steps.  A departure from the single-device
route: the TAILS ARE DROPPED — no short last batch, and the images a larger shard has beyond the smallest sit the epoch out.
The test set, eval, snapshots and the export live on replica 0; --resume and --init set replica 0 and broadcast.  --generate
with --devices is refused.  Without --devices the tool behaves to the byte as before.

python -m gpd_amd.train TRAIN_DIR ... --net F1,F2,H1[,H2]

trains a network of other widths — pytorch/network.py::Net with conv1_out F1, conv2_out F2 and fc1_out H1, or ::NetCCFFF with a
third dense layer of H2 outputs (train_net3.py's commented-out alternative) — with either recipe and with --devices; under
--recipe caffe it is that network without the ReLUs behind the convolutions.  The initial state is the seeded filler of the
recipe for those widths.  DIR receives what gpd_amd.torch_export writes for such a network — the 8 or 10 tensors in torch
layout and a network.cfg that names the widths (and conv_relu = 0 under the Caffe recipe) — and model.pwf holds the same
tensors; snapshots and --resume carry them all.  --init is refused (an Eigen-layout directory has the stock widths), and so is
--freeze with a third dense layer (the recipe has multipliers for eight tensors).  Without --net nothing changes.
"""
import argparse
import os
import sys

import numpy as np

from gpd_amd import api, eigen_export, torch_export


def load_set(directory, prefix, channels=None):
    img = np.load(os.path.join(directory, prefix + "_images.npy"))
    lab = np.load(os.path.join(directory, prefix + "_labels.npy")).reshape(-1)
    if img.ndim != 4 or img.shape[1:3] != (60, 60) or img.shape[0] != len(lab):
        raise ValueError("%s: %s_images.npy %s / %s_labels.npy %s are not [n,60,60,C] / [n]" % (directory, prefix, img.shape, prefix, lab.shape))
    if channels is not None and img.shape[3] != channels:
        raise ValueError("%s: %d channels, the training set has %d" % (directory, img.shape[3], channels))
    return np.ascontiguousarray(img, np.uint8), np.ascontiguousarray(lab, np.uint8)


def config_values(path):
    """The `key = value` lines of a generate_data configuration -> {key: value string}"""
    values = {}
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0]
            if "=" in line:
                k, v = line.split("=", 1)
                values[k.strip()] = v.strip()
    return values


def fill_sets(trainer, a, train_set=None):
    """The trainer's two resident sets, from --generate's configuration or from the .npy pairs -> (n, n_test)"""
    if a.generate:
        from gpd_amd import hostlib
        hostlib.generate_data(a.generate, trainer)
        return trainer.count(0)[0], trainer.count(1)[0]
    img, lab = train_set
    trainer.set_data(img, lab, 0)
    n_test = 0
    if a.test:
        timg, tlab = load_set(a.test, "test", img.shape[3])
        trainer.set_data(timg, tlab, 1)
        n_test = len(tlab)
    return len(lab), n_test


def open_sets(a):
    """-> (channels, device, the loaded training pair or None under --generate)"""
    if a.generate:
        cfg = config_values(a.generate)
        return int(cfg.get("image_num_channels", 15)), int(cfg.get("hip_device", a.device)), None
    train_set = load_set(a.train_dir, "train")
    return train_set[0].shape[3], a.device, train_set


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


TEST_INTERVAL, TEST_IMAGES = 100, 10000  # the solver file's test_interval; test_iter 100 of batches of 100


def batch_rows(seed, n, batch, first, count, per=None):
    """Rows first .. first + count of the endless list of full batches: pass e over the set is gpd_hip_shuffle_orders' order
    number e, cut into n // batch rows (Caffe's data layer wraps around; here every pass is shuffled and its tail dropped).
    per: rows taken from a pass where that is fewer than n // batch (a replica beside one with a smaller shard)."""
    per = n // batch if per is None else per
    if per < 1:
        raise ValueError("the training set has %d images, a batch needs %d" % (n, batch))
    e0, e1 = first // per, (first + count - 1) // per
    orders = api.shuffle_orders(seed, [n] * (e1 + 1))[e0:]
    rows = np.concatenate([o[:per * batch].reshape(per, batch) for o in orders])
    return rows[first - e0 * per:first - e0 * per + count]


def trainer_kw(a):
    """The Trainer arguments --net asks for"""
    return dict(shape=a.net) if a.net else {}


def write_snapshot(trainer, directory):
    os.makedirs(directory, exist_ok=True)
    s = trainer.get_solver_state()
    np.savez(os.path.join(directory, "state.npz"), **trainer.get_state())
    np.savez(os.path.join(directory, "solver.npz"), count=np.int64(s["count"]), **{"m." + k: v for k, v in s["m"].items()})


def read_snapshot(trainer, directory):
    """-> the iteration the snapshot was taken at"""
    with np.load(os.path.join(directory, "state.npz")) as z:
        trainer.set_state({k: z[k] for k in trainer.keys})
    with np.load(os.path.join(directory, "solver.npz")) as z:
        count = int(z["count"])
        trainer.set_solver_state(dict(count=count, m={k: z["m." + k] for k in trainer.keys}, v=None))
    return count


def replica_seed(seed, r):
    """The seed of replica r's orders"""
    return (int(seed) + 1000003 * (r + 1)) & 0xFFFFFFFF


def shard_steps(shards, batch):
    """Steps of an epoch over shards of these sizes at a batch of `batch` per replica: the smallest shard's full batches"""
    per = min(shards) // batch
    if per < 1:
        raise ValueError("the smallest shard has %d images, a replica's batch needs %d" % (min(shards), batch))
    return per


def train_group(group, shards, epochs, batch, seed, n_test=0, log=print):
    """train() over a TrainerGroup: `batch` is the global batch, shards the replicas' image counts -> replica 0's final state."""
    G = len(group)
    b = batch // G
    per = shard_steps(shards, b)
    orders = [api.shuffle_orders(replica_seed(seed, r), [shards[r]] * epochs) for r in range(G)]
    first = group.trainers[0]
    for epoch in range(epochs):
        losses, _ = group.steps(np.stack([orders[r][epoch][:per * b].reshape(per, b) for r in range(G)]))
        for i in range(999, len(losses), 1000):
            log("[%d, %5d] loss: %.3f" % (epoch + 1, i + 1, float(losses[i - 999:i + 1].mean())))
        if len(losses) % 1000:
            log("[%d, %5d] loss: %.3f" % (epoch + 1, len(losses), float(losses[len(losses) // 1000 * 1000:].mean())))
        if n_test:
            _, correct = first.eval(n=n_test, which=1)
            log("epoch: %d, correct: %d, total: %d, accuracy: %.3f" % (epoch + 1, correct, n_test, correct / n_test))
    return first.get_state()


def group_rows(seed, shards, batch, first, count):
    """batch_rows for every replica of a group (batch: per replica) -> i32 [G, count, batch]"""
    per = shard_steps(shards, batch)
    return np.stack([batch_rows(replica_seed(seed, r), n, batch, first, count, per) for r, n in enumerate(shards)])


def train_caffe(trainer, n, max_iter, batch, seed, n_test=0, start=0, snapshot=0, out=None, log=print, group=None):
    """Iterations start .. max_iter of the Caffe recipe over the trainer's resident sets -> the final state.  group: a
    TrainerGroup whose replica 0 is `trainer`; n is then the list of the replicas' image counts and batch the global batch."""
    n_test = min(TEST_IMAGES, n_test)
    it = start
    while it < max_iter:
        stop = min(max_iter, (it // TEST_INTERVAL + 1) * TEST_INTERVAL)
        if snapshot:
            stop = min(stop, (it // snapshot + 1) * snapshot)
        if group is None:
            losses = trainer.steps(batch_rows(seed, n, batch, it, stop - it))
        else:
            losses, _ = group.steps(group_rows(seed, n, batch // len(group), it, stop - it))
        it = stop
        if it % TEST_INTERVAL == 0 or it == max_iter:
            lr = float(api.learning_rate(trainer.recipe, trainer.params.lr, it - 1))
            line = "Iteration %d, lr = %.6g, loss = %.6g" % (it, lr, float(losses[-1]))
            if n_test:
                _, correct = trainer.eval(n=n_test, which=1)
                line += ", accuracy = %.4f" % (correct / n_test)
            log(line)
        if snapshot and it % snapshot == 0:
            write_snapshot(trainer, os.path.join(out, "snapshot_%d" % it))
    return trainer.get_state()


def frozen_names(spec):
    names = []
    for name in [s for s in spec.split(",") if s]:
        hit = [k for k in api.TORCH_KEYS if k == name or k.split(".")[0] == name]
        if not hit:
            raise ValueError("--freeze: no tensor %r (%s)" % (name, ", ".join(api.TORCH_KEYS)))
        names += hit
    return names


class Replicas:
    """--devices: a context and a trainer per listed device and the group over them, closed in order.  Replica r holds the
    training images r, r + G, ...; the test set lives on replica 0."""

    def __init__(self, a, train_set, **trainer_kw):
        img, lab = train_set
        C, G = img.shape[3], len(a.devices)
        self.ctxs, self.trainers, self.group = [], [], None
        try:
            for d in a.devices:
                self.ctxs.append(api.Context(api.default_params(C), device=d))
                self.trainers.append(api.Trainer(self.ctxs[-1], max_batch=a.batch // G, **trainer_kw))
            self.group = api.TrainerGroup(self.trainers)
            for r, t in enumerate(self.trainers):
                t.set_data(img[r::G], lab[r::G], 0)
            self.shards = [len(lab[r::G]) for r in range(G)]
            self.n_test = 0
            if a.test:
                timg, tlab = load_set(a.test, "test", C)
                self.trainers[0].set_data(timg, tlab, 1)
                self.n_test = len(tlab)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.group is not None:
            self.group.close()
        for t in self.trainers:
            t.close()
        for c in self.ctxs:
            c.close()


def main_caffe(a):
    C, device, train_set = open_sets(a)
    recipe = api.train_default_recipe(1, lr_mult={k: 0.0 for k in frozen_names(a.freeze or "")})
    reps = Replicas(a, train_set, recipe=recipe, lr=api.CAFFE_BASE_LR, **trainer_kw(a)) if a.devices else None
    if reps:
        ctx, trainer = None, reps.trainers[0]
    else:
        ctx = api.Context(api.default_params(C), device=device)
        trainer = api.Trainer(ctx, recipe=recipe, max_batch=a.batch, lr=api.CAFFE_BASE_LR, **trainer_kw(a))
    try:
        scale = float(trainer.params.input_scale)
        start = 0
        if a.resume:
            start = read_snapshot(trainer, a.resume)
        elif a.init:
            # a file the directory lacks (the reference's snapshot: ip1_weights.bin) starts from the xavier filler
            fill = api.lenet_from_torch(api.init_xavier(C, a.seed), C, scale)
            trainer.set_state(eigen_export.to_torch(eigen_export.load(a.init, fill), scale))
        else:
            trainer.set_state(api.init_xavier(C, a.seed, shape=a.net))
        if reps:
            reps.group.broadcast(0)
            n, n_test = sum(reps.shards), reps.n_test
            print("training on %d images of %d channels over %d replicas from iteration %d to %d%s"
                  % (n, C, len(reps.shards), start, a.max_iter, ", testing on %d" % min(TEST_IMAGES, n_test) if n_test else ""))
            state = train_caffe(trainer, reps.shards, a.max_iter, a.batch, a.seed, n_test, start, a.snapshot, a.out, group=reps.group)
        else:
            n, n_test = fill_sets(trainer, a, train_set)
            print("training on %d images of %d channels from iteration %d to %d%s" % (n, C, start, a.max_iter, ", testing on %d" % min(TEST_IMAGES, n_test) if n_test else ""))
            state = train_caffe(trainer, n, a.max_iter, a.batch, a.seed, n_test, start, a.snapshot, a.out)
        if a.net:  # the Eigen layout has the stock widths only
            names = torch_export.export(state, a.out, scale, conv_relu=False)
        else:
            names = eigen_export.export(state, a.out, scale)
    finally:
        if reps:
            reps.close()
        else:
            trainer.close()
            ctx.close()
    if a.net:
        names += save_pwf(state, a.out)
    print("wrote %s: %s" % (a.out, " ".join(names)))
    return 0


def save_pwf(state, out):
    """model.pwf, torch.save of the state dict as pytorch/train_net3.py saves it, where torch imports -> the names written"""
    try:
        import torch
    except ImportError:
        return []
    torch.save({k: torch.from_numpy(v.copy()) for k, v in state.items()}, os.path.join(out, "model.pwf"))
    return ["model.pwf"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gpd_amd.train", description="train the grasp network on the device")
    ap.add_argument("train_dir", nargs="?", help="directory with train_images.npy and train_labels.npy (generate_data)")
    ap.add_argument("--generate", metavar="CONFIG", help="a generate_data configuration: fill the resident sets on the device instead of reading TRAIN_DIR")
    ap.add_argument("--test", help="directory with test_images.npy and test_labels.npy")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0, help="of the initial state and of the epochs' orders")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--devices", help="train on several replicas: a comma-separated device list, one replica each (a device listed twice carries two)")
    ap.add_argument("--out", required=True, help="parameter directory to write")
    ap.add_argument("--recipe", choices=["torch", "caffe"], default="torch", help="caffe: the deployed LeNet under the reference's Caffe solver")
    ap.add_argument("--max-iter", type=int, default=10000, help="caffe: iterations (the solver file's max_iter)")
    ap.add_argument("--snapshot", type=int, default=0, help="caffe: write state and solver state every N iterations")
    ap.add_argument("--resume", help="caffe: a snapshot directory to continue from")
    ap.add_argument("--init", help="caffe: an Eigen-layout parameter directory to start from")
    ap.add_argument("--freeze", help="caffe: tensors or layers whose lr_mult is 0, comma-separated")
    ap.add_argument("--net", metavar="F1,F2,H1[,H2]", help="other widths: conv1_out, conv2_out, fc1_out and, for NetCCFFF, fc2_out")
    a = ap.parse_args(argv)
    if a.net is not None:
        try:
            a.net = tuple(int(x) for x in a.net.split(","))
        except ValueError:
            ap.error("--net takes three or four comma-separated widths")
        if len(a.net) not in (3, 4) or min(a.net) < 1:
            ap.error("--net takes three or four positive widths: F1,F2,H1[,H2]")
        if a.init:
            ap.error("--init reads an Eigen-layout directory, which has the stock widths: it goes without --net")
        if a.freeze and len(a.net) == 4:
            ap.error("--freeze with a third dense layer: the recipe has multipliers for eight tensors")
    if a.generate and (a.train_dir or a.test):
        ap.error("--generate fills both sets itself: it goes without TRAIN_DIR and --test")
    if not a.generate and not a.train_dir:
        ap.error("TRAIN_DIR or --generate CONFIG is needed")
    if a.recipe != "caffe" and (a.resume or a.init or a.freeze or a.snapshot):
        ap.error("--snapshot, --resume, --init and --freeze need --recipe caffe")
    if a.devices is not None:
        if a.generate:
            ap.error("--generate with --devices: generating over several devices is not there yet; write the set with generate_data and pass TRAIN_DIR")
        try:
            a.devices = [int(d) for d in a.devices.split(",")]
        except ValueError:
            ap.error("--devices takes a comma-separated list of device numbers")
        if not 1 <= len(a.devices) <= 16 or min(a.devices) < 0:
            ap.error("--devices takes 1 .. 16 device numbers")
        if a.batch % len(a.devices):
            ap.error("--batch %d is the global batch: it must be divisible by the %d replicas" % (a.batch, len(a.devices)))
    return a


def main(argv=None):
    a = parse_args(argv)
    if a.recipe == "caffe":
        return main_caffe(a)
    C, device, train_set = open_sets(a)
    reps = Replicas(a, train_set, **trainer_kw(a)) if a.devices else None
    if reps:
        ctx, trainer = None, reps.trainers[0]
    else:
        ctx = api.Context(api.default_params(C), device=device)
        trainer = api.Trainer(ctx, max_batch=a.batch, **trainer_kw(a))
    try:
        trainer.set_state(api.init_state(C, a.seed, shape=a.net))
        if reps:
            reps.group.broadcast(0)
            print("training on %d images of %d channels over %d replicas%s" % (sum(reps.shards), C, len(reps.shards), ", testing on %d" % reps.n_test if reps.n_test else ""))
            state = train_group(reps.group, reps.shards, a.epochs, a.batch, a.seed, reps.n_test)
        else:
            n, n_test = fill_sets(trainer, a, train_set)
            print("training on %d images of %d channels%s" % (n, C, ", testing on %d" % n_test if n_test else ""))
            state = train(trainer, n, a.epochs, a.batch, a.seed, n_test)
        names = torch_export.export(state, a.out, float(trainer.params.input_scale))
    finally:
        if reps:
            reps.close()
        else:
            trainer.close()
            ctx.close()
    names += save_pwf(state, a.out)
    print("wrote %s: %s" % (a.out, " ".join(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
