"""Drop-in for the reference CLI runners/torch_run_physics.py (:1-117).

Same flags, names, types, defaults and store_true/store_false semantics
(:10-34), same task table (:49-75), same train-then-test flow (:77-117);
the model is the HIP-backed PhysicsNet of this package.

Additive flags only:
  --loss_mode {fresh,reference}  fresh (default): the loss is the current
        forward's; reference: reproduce quirk Q1 (stale self.output).
  --data_dir DIR                 where <task file> lives (default: the
        reference's data/datasets relative to this runner, :86-89).
  --synthetic N                  if the task's npz is missing, render one with
        N training sequences (N//10 valid/test) with nn/datasets/synth.py.
  --seed S                       shared shuffle seed (required for DDP sharding).
  --device_data {1,0}            1 (default): uint8 dataset resident in HBM, each
        batch gathered on the GPU; 0: the reference's host path.
  --clip_grad_norm X             clip the global gradient norm to X before the update
        (torch's clip_grad_norm_ rule, taken on the device; 0 = off, the default).
  --physics_lr_mult M            the physics parameters (rollout_cell.*) step with
        base_lr * M (default 1).
  --log_grad_norms               total and per-group gradient norms on the train lines,
        a warning when a group's gradients are exactly zero.
  --physics_2d                   two objects in the plane: spring_color, spring_color_half,
        mnist_spring_color and bouncing_balls roll out with spring2d_ode_cell / bouncing2d_ode_cell
        (the cells with split size 2: a vector spring between (x0, y0) and (x1, y1); four walls)
        instead of the reference's split-size-1 cells (quirk Q3).  Off by default; the
        state_dict is the same, so checkpoints move between the two.  An error for 3bp_color.
  --blackbox_dynamics            the black-box baseline: every task rolls out with lstm_ode_cell
        (nn.LSTMCell of --recurrent_units hidden units + a linear read-out, on the device) instead
        of its physics cell.  Off by default; an error together with --physics_2d.
  --interaction_dynamics         the object-centric learned baseline: every task rolls out with
        interaction_ode_cell (an interaction network: one relation MLP over all ordered pairs of
        objects, one object MLP, --recurrent_units hidden units, on the device) instead of its
        physics cell.  Off by default; an error together with --blackbox_dynamics or --physics_2d.
  --synthetic_device {0,1}       1: with --synthetic N and the task's npz missing,
        render the data on the GPU instead (nn/datasets/synth_device.py: HIP
        integrators + rasteriser) and keep it in HBM; no npz is written.  Same
        distribution as synth.py, other sequences.  Under data parallelism every
        rank renders the same dataset and takes its shard.  0 (default): as before.
  --synthetic_stream {0,1}       1: with --synthetic N and --device_data 1, the training split
        is an unlimited stream rendered on the GPU while the previous step runs
        (StreamingDeviceIterator: two batches of HBM, no batch seen twice, N the nominal
        epoch size; under data parallelism every rank streams its own data).  Valid and test
        are rendered once on the device (N//10 each) and stay resident.  Nothing is read
        from or written to --data_dir; the stream's statistics are logged at every
        evaluation.  0 (default): as before.

Data-parallel training: launch with torchrun (one process per GPU, RCCL);
--batch_size is per rank, every rank draws a disjoint shard of each epoch.

    PYTHONPATH=. python runners/torch_run_physics.py --task spring_color --color \\
        --autoencoder_loss 3.0 --save_dir /tmp/run --synthetic 2000
"""
import argparse
import logging
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from paig_reproduction_amd.nn.network import physics_models  # noqa: E402
from paig_reproduction_amd.nn.utils.misc import classes_in_module  # noqa: E402
from paig_reproduction_amd.nn.datasets.iterators import get_iterators  # noqa: E402

TASKS = {
    # task: (train file, test file, cell, seq_len, test_seq_len, input_steps, pred_steps, input_size)
    "bouncing_balls": ("bouncing/color_bounce_vx8_vy8_sl12_r2.npz", "bouncing/color_bounce_vx8_vy8_sl30_r2.npz",
                       "bouncing_ode_cell", 12, 30, 4, 6, 32 * 32),
    "spring_color": ("spring_color/color_spring_vx8_vy8_sl12_r2_k4_e6.npz",
                     "spring_color/color_spring_vx8_vy8_sl30_r2_k4_e6.npz", "spring_ode_cell", 12, 30, 4, 6, 32 * 32),
    "spring_color_half": ("spring_color_half/color_spring_vx4_vy4_sl12_r2_k4_e6_halfpane.npz",
                          "spring_color_half/color_spring_vx4_vy4_sl30_r2_k4_e6_halfpane.npz", "spring_ode_cell",
                          12, 30, 4, 6, 32 * 32),
    "3bp_color": ("3bp_color/color_3bp_vx2_vy2_sl20_r2_g60_m1_dt05.npz",
                  "3bp_color/color_3bp_vx2_vy2_sl40_r2_g60_m1_dt05.npz", "gravity_ode_cell", 20, 40, 4, 12, 36 * 36),
    "mnist_spring_color": ("mnist_spring_color/color_mnist_spring_vx8_vy8_sl12_r2_k2_e12.npz",
                           "mnist_spring_color/color_mnist_spring_vx8_vy8_sl30_r2_k2_e12.npz", "spring_ode_cell",
                           12, 30, 3, 7, 64 * 64),
}


def build_parser():
    p = argparse.ArgumentParser(description="PyTorch version of the TensorFlow script.")
    p.add_argument("--epochs", type=int, default=10, help="Number of epochs to train")
    p.add_argument("--batch_size", type=int, default=100, help="Training batch size (per rank)")
    p.add_argument("--save_dir", type=str, default="", help="Directory to save checkpoint and logs")
    p.add_argument("--use_ckpt", action="store_true", help="Whether to start from scratch or start from checkpoint")
    p.add_argument("--ckpt_dir", type=str, default="", help="Checkpoint directory to use")
    p.add_argument("--base_lr", type=float, default=1e-3, help="Base learning rate")
    p.add_argument("--anneal_lr", action="store_false", help="Whether to anneal lr after 0.75 of total epochs")
    p.add_argument("--optimizer", type=str, default="rmsprop", help="Optimizer to use")
    p.add_argument("--save_every_n_epochs", type=int, default=5, help="Epochs between checkpoint saves")
    p.add_argument("--eval_every_n_epochs", type=int, default=1, help="Epochs between validation run")
    p.add_argument("--print_interval", type=int, default=10, help="Print train metrics every n mini-batches")
    p.add_argument("--debug", action="store_true", help="If true, eval is not run before training")
    p.add_argument("--test_mode", action="store_true", help="If true, only run test set")
    p.add_argument("--task", type=str, default="", help="Type of task.")
    p.add_argument("--model", type=str, default="PhysicsNet", help="Model to use.")
    p.add_argument("--recurrent_units", type=int, default=100,
                   help="Number of units for each lstm, if using black-box dynamics.")
    p.add_argument("--lstm_layers", type=int, default=1,
                   help="Number of lstm cells to use, if using black-box dynamics")
    p.add_argument("--cell_type", type=str, default="", help="Type of pendulum to use.")
    p.add_argument("--encoder_type", type=str, default="conv_encoder", help="Type of encoder to use.")
    p.add_argument("--decoder_type", type=str, default="conv_st_decoder", help="Type of decoder to use.")
    p.add_argument("--autoencoder_loss", type=float, default=0.0, help="Autoencoder loss weighing.")
    p.add_argument("--alt_vel", action="store_true", help="Whether to use linear velocity computation.")
    p.add_argument("--color", action="store_true", help="Whether images are RGB or grayscale.")
    p.add_argument("--datapoints", type=int, default=0,
                   help="How many datapoints from the dataset to use. Default=0 uses all data.")
    # additive
    p.add_argument("--loss_mode", choices=("fresh", "reference"), default="fresh")
    p.add_argument("--data_dir", type=str, default=os.path.join(REPO, "data", "datasets"))
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32",
                   help="fp32: fp32-accurate results (convs/GEMMs on the 16-bit matrix cores with split "
                        "hi+lo operands); bf16: bf16 operands, fp32 accumulation (BASELINE config #2)")
    p.add_argument("--conv_math", choices=("split", "fp32", "bf16"), default=None,
                   help="override the conv/GEMM arithmetic directly (fp32 = f32-input MFMA)")
    p.add_argument("--device_data", type=int, default=1,
                   help="1: dataset resident in HBM as uint8, batches gathered on the GPU (F2); 0: host iterators")
    p.add_argument("--synthetic_device", type=int, choices=(0, 1), default=0,
                   help="1: render a missing --synthetic dataset on the GPU and keep it there (no npz written)")
    p.add_argument("--synthetic_stream", type=int, choices=(0, 1), default=0,
                   help="1: stream never-repeating training batches from the device renderer (needs --synthetic N, "
                        "the nominal epoch size, and --device_data 1); nothing touches --data_dir")
    p.add_argument("--sigma", type=float, default=1.0,
                   help="decoder attention-window scale (PhysicsNet.log_sig), in [0.5, 2]: 2 halves the window")
    p.add_argument("--learn_sigma", action="store_true",
                   help="train the decoder attention-window scale on the device (sigma = exp(ln 2 tanh(u)), one "
                        "extra parameter decoder_sigma_u); --sigma is its start value, strictly inside (0.5, 2)")
    p.add_argument("--clip_grad_norm", type=float, default=0.0,
                   help="clip the global gradient norm to this value before the update (0: off)")
    p.add_argument("--physics_lr_mult", type=float, default=1.0,
                   help="learning rate of the physics parameters (rollout_cell.*), as a multiple of --base_lr")
    p.add_argument("--log_grad_norms", action="store_true",
                   help="log the total and per-group gradient norms on the train lines")
    p.add_argument("--physics_2d", action="store_true",
                   help="two objects in the plane: the task's spring / bouncing cell with split size 2 (a vector "
                        "spring, four walls) instead of the reference's split-size-1 cell; not for 3bp_color")
    p.add_argument("--blackbox_dynamics", action="store_true",
                   help="the black-box baseline: every task rolls out with lstm_ode_cell (an LSTM of "
                        "--recurrent_units hidden units and a linear read-out) instead of its physics cell; "
                        "not with --physics_2d")
    p.add_argument("--interaction_dynamics", action="store_true",
                   help="the object-centric learned baseline: every task rolls out with interaction_ode_cell (an "
                        "interaction network of --recurrent_units hidden units) instead of its physics cell; not "
                        "with --blackbox_dynamics or --physics_2d")
    return p


# --physics_2d: the task's preset cell -> its split-size-2 class
CELLS_2D = {"spring_ode_cell": "spring2d_ode_cell", "bouncing_ode_cell": "bouncing2d_ode_cell"}


def task_cell(args):
    """The rollout cell of args.task: TASKS' preset, or under --physics_2d its
    2-D class (an error for a task whose cell has none), or under
    --blackbox_dynamics / --interaction_dynamics the learned lstm_ode_cell /
    interaction_ode_cell for every task."""
    if getattr(args, "interaction_dynamics", False):
        if getattr(args, "blackbox_dynamics", False) or args.physics_2d:
            raise SystemExit("--interaction_dynamics replaces the physics cell: it cannot be combined with "
                             "--blackbox_dynamics or --physics_2d")
        return "interaction_ode_cell"
    if getattr(args, "blackbox_dynamics", False):
        if args.physics_2d:
            raise SystemExit("--blackbox_dynamics replaces the physics cell: it cannot be combined with --physics_2d")
        return "lstm_ode_cell"
    cell = TASKS[args.task][2]
    if not args.physics_2d:
        return cell
    if cell not in CELLS_2D:
        raise SystemExit(f"--physics_2d: task {args.task} ({cell}) has no 2-D cell; it applies to " +
                         ", ".join(t for t, v in TASKS.items() if v[2] in CELLS_2D))
    return CELLS_2D[cell]


def dataset_path(args, rel, seq_len):
    path = os.path.join(args.data_dir, rel)
    if not os.path.exists(path) and args.synthetic > 0:
        from paig_reproduction_amd.nn.datasets.synth import write_dataset
        if _rank() == 0:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            n = args.synthetic
            write_dataset(path, args.task, seq_len, n, max(n // 10, 1), max(n // 10, 1), seed=0)
        if dist.is_initialized():
            dist.barrier()
    return path


def _rank():
    return dist.get_rank() if dist.is_initialized() else 0


def iterators(args, rel, seq_len, rank, world, device, train=True):
    """The task's train / valid / test iterators for sequences of seq_len
    (train=False: the test pass, which reads the test split only)."""
    if args.synthetic_stream:
        from paig_reproduction_amd.nn.datasets.synth_device import streaming_iterators
        n = args.synthetic
        return streaming_iterators(args.task, seq_len, args.batch_size, n, max(n // 10, 1), max(n // 10, 1), args.seed,
                                   device, rank=rank, world=world, data_seed=0, stream=train)
    if args.synthetic_device and args.synthetic > 0 and not os.path.exists(os.path.join(args.data_dir, rel)):
        from paig_reproduction_amd.nn.datasets.synth_device import device_iterators
        n = args.synthetic
        return device_iterators(args.task, seq_len, n, max(n // 10, 1), max(n // 10, 1), args.seed, device,
                                rank=rank, world=world, data_seed=0)
    return get_iterators(dataset_path(args, rel, seq_len), conv=True, datapoints=args.datapoints,
                         seed=args.seed, rank=rank, world=world, device=device if args.device_data else None)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.synthetic_stream and not (args.synthetic > 0 and args.device_data):
        raise SystemExit("--synthetic_stream 1 needs --synthetic N (the epoch size) and --device_data 1")
    logger = logging.getLogger("torch")
    logger.setLevel(logging.DEBUG)
    if not logger.handlers:
        ch = logging.StreamHandler()
        ch.setLevel(logging.DEBUG)
        ch.setFormatter(logging.Formatter('%(asctime)s - %(name)s - %(message)s'))
        logger.addHandler(ch)

    Model = classes_in_module(physics_models)[args.model]
    data_file, test_data_file, cell_type, seq_len, test_seq_len, input_steps, pred_steps, input_size = \
        TASKS[args.task]
    cell_type = task_cell(args)   # the training model and the test-time model alike
    if args.blackbox_dynamics and args.physics_lr_mult != 1.0:
        logger.warning("--physics_lr_mult %g has no effect with --blackbox_dynamics: lstm_ode_cell has no fp64 "
                       "physics parameter, its weights step with --base_lr", args.physics_lr_mult)
    if args.interaction_dynamics and args.physics_lr_mult != 1.0:
        logger.warning("--physics_lr_mult %g has no effect with --interaction_dynamics: interaction_ode_cell has no "
                       "fp64 physics parameter, its weights step with --base_lr", args.physics_lr_mult)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("paig_reproduction_amd trains on the GPU only (HIP kernels); no CUDA/ROCm device found")
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        if args.seed is None:
            args.seed = 0   # every rank must shuffle with the same permutation
    device = torch.device(f"cuda:{local}")
    rank = _rank()

    def make(sl):
        if args.seed is not None:
            torch.manual_seed(args.seed)
        net = Model(args.task, args.recurrent_units, args.lstm_layers, cell_type, sl, input_steps, pred_steps,
                    args.autoencoder_loss, args.alt_vel, args.color, input_size, args.encoder_type,
                    args.decoder_type, device=device, sigma=args.sigma, learn_sigma=args.learn_sigma)
        net.loss_mode = args.loss_mode
        net.conv_math = args.conv_math or ("bf16" if args.dtype == "bf16" else "split")
        net.to(net.device)
        if world > 1:
            for t in net.state_dict().values():
                dist.broadcast(t, 0)
        return net

    optim = {"max_grad_norm": args.clip_grad_norm, "physics_lr_mult": args.physics_lr_mult,
             "grad_norms": args.log_grad_norms}
    if not args.test_mode:
        network = make(seq_len)
        its = iterators(args, data_file, seq_len, rank, world, device)
        network.get_data(its)
        network.build_optimizer(args.base_lr, args.optimizer, args.anneal_lr, **optim)
        network.initialize_graph(args.save_dir, args.use_ckpt, args.ckpt_dir)
        network.train_model(args.epochs, args.batch_size, args.save_every_n_epochs, args.eval_every_n_epochs,
                            args.print_interval, args.debug)

    network = make(test_seq_len)
    network.build_optimizer(args.base_lr, args.optimizer, args.anneal_lr, **optim)
    network.initialize_graph(args.save_dir, True, args.ckpt_dir)
    its = iterators(args, test_data_file, test_seq_len, rank, world, device, train=False)
    network.get_data(its)
    network.train_model(0, args.batch_size, args.save_every_n_epochs, args.eval_every_n_epochs,
                        args.print_interval, args.debug)
    if world > 1:
        dist.destroy_process_group()
    return network


if __name__ == "__main__":
    main()
