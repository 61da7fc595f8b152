#!/usr/bin/env python3
"""Track-X benchmark (NOT the BASELINE metric -- that is bench.py): training images/s of the trainable convolution
network BASELINE.json's north_star asks for, on the configs SURVEY.md §8(d) fixes:

  cifar   CIFAR-10 shape 32x32x3: conv3x3 3->32, pool, 32->64, pool, 64->128, pool -> 2048 -> 256 -> 10, B = 512   (configs[2])
  synth224  synthetic 224x224x3, 8 conv layers, 128 images per GPU (global batch 1024 on 8 GPUs)                    (configs[3])
  mnist   MNIST shape 28x28x1 LeNet-style: conv 1->32, pool, conv 32->64, pool -> 3136 -> 128 -> 10, B = 256      (configs[1], trainable form)
  cifar_bn  cifar with every conv + ReLU written Conv2d -> BatchNorm2d -> ReLU: ("conv_linear", n), ("bn_relu",) (not bf16_stored)
  cifar_res cifar_bn with a basic residual block (identity shortcut) behind each conv_linear, bn_relu pair: ... ("bn_add_relu", 4)
  cifar_res_gap  cifar_res ending as a ResNet does: its last pool and the 2048 -> 256 dense layer replaced by ("global_avgpool",), 8x8x128 -> 128 -> 10
  cifar_resnet14  the CIFAR ResNet of 6n + 2 layers (He et al., section 4.2, option-A shortcuts), n = 2, at widths 32 / 64 / 128: stride-2
                  convolutions and ("bn_add_relu_down", 4) shortcuts between the stages, no pool; 27 layers with parameters, B = 512
  cifar_bottleneck  bottleneck residual blocks on ("conv1x1_linear", C) layers: conv_linear 128, bn_relu; two blocks of width 128 (1x1 to 32,
                  3x3 at 32, 1x1 to 128, ("bn_add_relu", 6)); pool; conv1x1_linear 256, bn_relu; two blocks of width 256; pool, global_avgpool,
                  dense 10; 29 layers with parameters, B = 512; --set pw=1 runs the 1x1 layers on the streaming kernel k_pw
  cifar_sep       depthwise-separable layers on ("dwconv_linear",) and ("conv1x1_linear", C): conv_linear 64, bn_relu; a residual separable
                  block at 64, a separable layer to 128, pool; the same at 128 and to 256, pool; two residual separable blocks at 256;
                  global_avgpool, dense 10; 27 layers with parameters, B = 512
  cifar_mbv2      MobileNetV2's inverted residual blocks (expansion 6) on ("dwconv_linear",), ("dwconv_linear_s2",), ("bn",) and ("bn_add", 6):
                  a stem of two conv_linear 32, bn_relu pairs; blocks 32 -> 32 (skip), 32 -> 64 stride 2, 64 -> 64 (skip), 64 -> 128 stride 2;
                  conv1x1_linear 256, bn_relu, global_avgpool, dense 10; 31 layers with parameters, B = 512

fp32 activations / weights, fp32 MFMA (v_mfma_f32_32x32x2_f32; peak 157.3 TFLOP/s).  Reports achieved TFLOP/s of the whole
training step (algorithmic 2*MACs of forward + dgrad + wgrad) and its fraction of the fp32 MFMA peak.  The reference has no
trainable convolution, so there is no reference number to compare with."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np

CONFIGS = {
    "cifar": ((32, 32, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("conv", 128), ("pool",), ("dense_relu", 256), ("dense", 10)), 512),
    "mnist": ((28, 28, 1), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 128), ("dense", 10)), 256),
    # configs[3]: synthetic 224x224x3, 8 conv layers (3->32->32 | 64->64 | 128->128 | 256->256, pool after each pair) -> 10;
    # global batch 1024 over 8 GPUs = 128 images per GPU (the per-GPU batch below; --gpus N runs N such shards)
    "synth224": ((224, 224, 3), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("conv", 64), ("pool",), ("conv", 128), ("conv", 128), ("pool",),
                                 ("conv", 256), ("conv", 256), ("pool",), ("dense", 10)), 128),
}
# the CIFAR net as torch writes it, Conv2d -> BatchNorm2d -> ReLU: every ("conv", n) is ("conv_linear", n), ("bn_relu",)
CONFIGS["cifar_bn"] = (CONFIGS["cifar"][0], tuple(m for l in CONFIGS["cifar"][1] for m in ((("conv_linear", l[1]), ("bn_relu",)) if l[0] == "conv" else (l,))), CONFIGS["cifar"][2])
# cifar_bn with one basic residual block of the stage's width behind each of its three conv_linear, bn_relu pairs, in front of the pool:
# conv_linear n, bn_relu, conv_linear n, ("bn_add_relu", 4) -- relu(bn(conv(relu(bn(conv(x))))) + x), x the pair's output four layers back
CONFIGS["cifar_res"] = (CONFIGS["cifar"][0], tuple(m for l in CONFIGS["cifar"][1] for m in ((("conv_linear", l[1]), ("bn_relu",), ("conv_linear", l[1]), ("bn_relu",), ("conv_linear", l[1]),
                                                                                                  ("bn_add_relu", 4)) if l[0] == "conv" else (l,))), CONFIGS["cifar"][2])
# cifar_res with a ResNet's ending: global average pooling over the last stage's 8x8x128 map in place of the last pool and the hidden dense
# layer, in front of a 128 x 10 logits layer
_res, _last_pool = CONFIGS["cifar_res"][1], max(i for i, l in enumerate(CONFIGS["cifar_res"][1]) if l[0] == "pool")
CONFIGS["cifar_res_gap"] = (CONFIGS["cifar"][0], _res[:_last_pool] + (("global_avgpool",),) + tuple(l for l in _res[_last_pool + 1:] if l[0] != "dense_relu"), CONFIGS["cifar"][2])
# The CIFAR ResNet of 6n + 2 layers with n = 2 (widths 32 / 64 / 128: widths are multiples of 32): conv_linear 32, bn_relu; two identity
# blocks at 32x32x32; a down block (conv_linear_s2 64, bn_relu, conv_linear 64, bn_add_relu_down 4) and one identity block at 16x16x64; the
# same at 8x8x128; global_avgpool, dense 10.  27 layers with parameters (the job tables take 32; ResNet-20 would need 39).
_block = lambda c: (("conv_linear", c), ("bn_relu",), ("conv_linear", c), ("bn_add_relu", 4))
_down = lambda c: (("conv_linear_s2", c), ("bn_relu",), ("conv_linear", c), ("bn_add_relu_down", 4))
CONFIGS["cifar_resnet14"] = (CONFIGS["cifar"][0], (("conv_linear", 32), ("bn_relu",)) + _block(32) + _block(32) + _down(64) + _block(64) + _down(128) + _block(128) +
                             (("global_avgpool",), ("dense", 10)), CONFIGS["cifar"][2])
# A bottleneck net at the CIFAR shape: conv_linear 128, bn_relu; two bottleneck blocks of width 128 (conv1x1_linear 32, bn_relu, conv_linear 32,
# bn_relu, conv1x1_linear 128, ("bn_add_relu", 6)); pool; a plain widening conv1x1_linear 256, bn_relu; two bottleneck blocks of width 256;
# pool, global_avgpool, dense 10.  29 layers with parameters.
_bottleneck = lambda c: (("conv1x1_linear", c // 4), ("bn_relu",), ("conv_linear", c // 4), ("bn_relu",), ("conv1x1_linear", c), ("bn_add_relu", 6))
CONFIGS["cifar_bottleneck"] = (CONFIGS["cifar"][0], (("conv_linear", 128), ("bn_relu",)) + _bottleneck(128) + _bottleneck(128) + (("pool",), ("conv1x1_linear", 256), ("bn_relu",)) +
                               _bottleneck(256) + _bottleneck(256) + (("pool",), ("global_avgpool",), ("dense", 10)), CONFIGS["cifar"][2])
# A depthwise-separable net at the CIFAR shape: conv_linear 64, bn_relu; a residual separable block (dwconv_linear, bn_relu, conv1x1_linear C,
# ("bn_add_relu", 4)) at 64 and a separable layer (dwconv_linear, bn_relu, conv1x1_linear C', bn_relu) to 128; pool; the same at 128 and to 256;
# pool; two residual separable blocks at 256; global_avgpool, dense 10.  27 layers with parameters.
_sep = lambda c: (("dwconv_linear",), ("bn_relu",), ("conv1x1_linear", c), ("bn_relu",))
_sep_res = lambda c: (("dwconv_linear",), ("bn_relu",), ("conv1x1_linear", c), ("bn_add_relu", 4))
CONFIGS["cifar_sep"] = (CONFIGS["cifar"][0], (("conv_linear", 64), ("bn_relu",)) + _sep_res(64) + _sep(128) + (("pool",),) + _sep_res(128) + _sep(256) + (("pool",),) +
                        _sep_res(256) + _sep_res(256) + (("global_avgpool",), ("dense", 10)), CONFIGS["cifar"][2])
# An inverted-residual net at the CIFAR shape, expansion 6: a stem of two conv_linear 32, bn_relu pairs (two 3x3 layers: every config here
# has at least two forward launches of the 3x3 / pool families, which tests/test_convnet_epoch_plan.py asks of each); four blocks
# conv1x1_linear 6C, bn_relu, dwconv_linear[_s2], bn_relu, conv1x1_linear C', then ("bn_add", 6) where the block keeps shape and width (stride 1,
# C' = C: the skip, no ReLU behind the sum) or ("bn",) where it does not: 32 -> 32, 32 -> 64 stride 2, 64 -> 64 (its source is the second
# block's bn), 64 -> 128 stride 2; the head conv1x1_linear 256, bn_relu, global_avgpool, dense 10.  31 layers with parameters (the job tables take 32).
_inverted = lambda c, co, s2: (("conv1x1_linear", 6 * c), ("bn_relu",), ("dwconv_linear_s2",) if s2 else ("dwconv_linear",), ("bn_relu",), ("conv1x1_linear", co),
                               ("bn",) if s2 or co != c else ("bn_add", 6))
CONFIGS["cifar_mbv2"] = (CONFIGS["cifar"][0], (("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_relu",)) + _inverted(32, 32, False) + _inverted(32, 64, True) + _inverted(64, 64, False) + _inverted(64, 128, True) +
                         (("conv1x1_linear", 256), ("bn_relu",), ("global_avgpool",), ("dense", 10)), CONFIGS["cifar"][2])
F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD
BF16_MFMA_PEAK_TFLOPS = 2516.8    # same guide: dense bf16 MFMA = 16x the fp32 MFMA rate (~2.5 PFLOP/s; never the 2:1-sparsity figure)
HBM_PEAK_GBS = 8000.0


def resident_set_figures(net, args, in_shape, B, lr):
    """--dataset N: whole epochs of train_epoch over a resident synthetic set (a fresh device permutation per epoch, its range check and
    the gather included), then evaluate over the set.  Whole-call rates from a host clock around work that ends in a synchronise.
    --lr-schedule / --augment: the same epochs once more as that recipe -- a warm-up + cosine rate per step from a device tensor, the
    gather through a random crop and flip -- timed the same way, beside the plain figure.
    --label-smoothing / --mix: those recipe epochs a third time with the smoothed loss and / or mixup / CutMix records (mix_plan, made and
    moved to the device before the clock starts), beside the recipe figure: mix_epoch_ms_per_step.
    --ema: the evaluation once more on the average of the parameters (two exchange launches per call), beside the live figures.
    --accumulate K: B is the micro-batch and an epoch is a whole number of cycles (N // B rounded down to a multiple of K); the recipe's
    schedule has one rate per UPDATE, repeated for the K micro-steps of its cycle."""
    import torch
    N = args.dataset
    K = args.accumulate
    nb = N // B // K * K
    if nb < 1:
        sys.exit(f"--dataset {N}: smaller than one batch of {B}" + (f" times --accumulate {K}" if K > 1 else ""))

    def schedule():
        """the recipe's rate per micro-step: warm-up + cosine over the epoch's updates, as a device tensor (or the constant rate)"""
        from mercer_research_amd.convnet import warmup_cosine
        if args.lr_schedule != "warmup_cosine":
            return lr
        updates = nb // K
        return torch.from_numpy(np.repeat(warmup_cosine(updates, lr, max(1, updates // 20)), K)).to(net.device)
    gen = torch.Generator(device=net.device).manual_seed(1)
    with torch.cuda.stream(net.stream):
        if args.config == "synth224":
            X = torch.randn((N,) + tuple(in_shape), generator=gen, device=net.device, dtype=torch.float32)
        else:
            X = torch.randint(0, 256, (N,) + tuple(in_shape), generator=gen, device=net.device, dtype=torch.uint8)
        Y = torch.randint(0, 10, (N,), generator=gen, device=net.device, dtype=torch.int32)
        losses = torch.zeros(nb, dtype=torch.float32, device=net.device)

        def epoch():
            perm = torch.randperm(N, generator=gen, device=net.device).int()
            net.train_epoch(X, Y, perm, B, lr, n_batches=nb, losses=losses)

        epoch()                                            # the first step of the first epoch instantiates the (B, lr) graph
        net.synchronize()
        epochs = max(1, -(-args.steps // nb))
        t0 = time.perf_counter()
        for _ in range(epochs):
            epoch()
        net.synchronize()
        el = time.perf_counter() - t0
        recipe = {}
        if args.lr_schedule != "none" or args.augment >= 0:
            from mercer_research_amd.convnet import Augment
            sched = schedule()
            seen = [0]

            def recipe_epoch():
                perm = torch.randperm(N, generator=gen, device=net.device).int()
                net.train_epoch(X, Y, perm, B, sched, n_batches=nb, losses=losses, augment=Augment(args.augment, True, 1, seen[0]) if args.augment >= 0 else None)
                seen[0] += 1

            recipe_epoch()                                 # a scheduled rate has its own graph: instantiated here, once
            net.synchronize()
            t0 = time.perf_counter()
            for _ in range(epochs):
                recipe_epoch()
            net.synchronize()
            rel = time.perf_counter() - t0
            recipe = {"recipe": {"lr_schedule": args.lr_schedule, "augment_pad": args.augment if args.augment >= 0 else None, "hflip": args.augment >= 0},
                      "recipe_epoch_ms_per_step": round(rel / (epochs * nb) * 1e3, 4)}
        if args.label_smoothing > 0 or args.mix != "none":
            from mercer_research_amd.convnet import Augment, mix_plan
            sched = schedule()
            alphas = {"mixup": (0.8, 0.0), "cutmix": (0.0, 1.0), "both": (0.8, 1.0)}.get(args.mix)
            plans = [net.mix_to_device(mix_plan(nb, in_shape[0], in_shape[1], alphas[0], alphas[1], seed=e)) for e in range(epochs + 1)] if alphas else None
            net.set_loss(args.label_smoothing)
            done = [0]

            def mix_epoch():
                perm = torch.randperm(N, generator=gen, device=net.device).int()
                net.train_epoch(X, Y, perm, B, sched, n_batches=nb, losses=losses, augment=Augment(args.augment, True, 2, done[0]) if args.augment >= 0 else None,
                                mix=plans[done[0]] if plans else None)
                done[0] += 1

            mix_epoch()                                    # pair labels (and a new loss setting) have their own graph: instantiated here, once
            net.synchronize()
            t0 = time.perf_counter()
            for _ in range(epochs):
                mix_epoch()
            net.synchronize()
            mel = time.perf_counter() - t0
            net.set_loss(0.0)                              # the figures below are those of the plain loss, as without these flags
            recipe.update({"mix": {"label_smoothing": args.label_smoothing, "mix": args.mix, "mixup_alpha": alphas[0] if alphas else None,
                                   "cutmix_alpha": alphas[1] if alphas else None},
                           "mix_epoch_ms_per_step": round(mel / (epochs * nb) * 1e3, 4)})
        graphs = net.graphs_instantiated()                 # read here: the trap below instantiates one per step on purpose
        if args.trap:
            # what the scheduled path removes: the same kind of schedule as one-batch calls with a new float rate each -- the rate is part
            # of a constant-rate graph's key, so every step pays an eager step, a capture and an instantiate
            from mercer_research_amd.convnet import warmup_cosine
            rates = [float(v) + 1e-6 for v in warmup_cosine(nb, lr, max(1, nb // 20))]
            perm = torch.randperm(N, generator=gen, device=net.device).int()
            net.synchronize()
            t0 = time.perf_counter()
            for s, rate in enumerate(rates):
                net.train_epoch(X, Y, perm, B, rate, n_batches=1, first_batch=s)
            net.synchronize()
            recipe.update({"trap_ms_per_step": round((time.perf_counter() - t0) / nb * 1e3, 4), "trap_graphs_instantiated": net.graphs_instantiated() - graphs})
        net.evaluate(X, Y)
        reps = max(1, -(-args.steps * B // (4 * N)))       # about a quarter of the timed steps' images
        t0 = time.perf_counter()
        for _ in range(reps):
            loss_sum, correct, _ = net.evaluate_async(X, Y, want_pred=False)
        net.synchronize()
        ev = time.perf_counter() - t0
        metrics = {}
        if args.eval_metrics:
            # the same pass once more through evaluate_metrics (k_eval_metrics in the place of k_eval_ce): top-1 / top-5 counts, confusion on
            topk = (1, 5) if net.classes >= 5 else (1,)
            net.evaluate_metrics(X, Y, topk=topk)
            t0 = time.perf_counter()
            for _ in range(reps):
                m = net.evaluate_metrics_async(X, Y, topk=topk, confusion=True)
            net.synchronize()
            metrics = {"eval_ms": round(ev / reps * 1e3, 4), "eval_metrics_ms": round((time.perf_counter() - t0) / reps * 1e3, 4),
                       "eval_top5": int(m["topk_correct"][1].item()) if len(topk) > 1 else None}
        ema = {}
        if args.ema > 0:
            net.evaluate(X, Y, weights="ema")
            t0 = time.perf_counter()
            for _ in range(reps):
                ema_loss_sum, ema_correct, _ = net.evaluate_async(X, Y, want_pred=False, weights="ema")
            net.synchronize()
            ema = {"eval_ema_images_per_s": round(reps * N / (time.perf_counter() - t0), 1), "eval_ema_mean_loss": round(float(ema_loss_sum.item()) / N, 4),
                   "eval_ema_correct": int(ema_correct.item())}
    return {"dataset": N, "dataset_dtype": str(X.dtype).replace("torch.", ""), "epochs_timed": epochs, "epoch_ms_per_step": round(el / (epochs * nb) * 1e3, 4), **recipe,
            "epoch_images_per_s": round(epochs * nb * B / el, 1), "eval_images_per_s": round(reps * N / ev, 1),
            "eval_mean_loss": round(float(loss_sum.item()) / N, 4), "eval_correct": int(correct.item()), **metrics, **ema, "graphs_instantiated": graphs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS), default="cifar")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0, help="images per GPU")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "bf16", "bf16_stored"], default="fp32",
                    help="GEMM operand precision of forward / dgrad: fp32 MFMA, bf16 MFMA with fp32 accumulate / storage / update, or bf16 MFMA with the "
                         "convolutional stage's activations and gradients also STORED as bf16 (RCN_HIPX_BF16_STORED)")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="a kernel-selection option of the net (rcn_hipx_set_option), e.g. fuse_pool_bwd=0; repeatable")
    ap.add_argument("--force-dp", action="store_true", help="run the data-parallel step (gradients -> all-reduce -> apply) even at one GPU: a group of one over RCCL")
    ap.add_argument("--dp-graph", type=int, default=1, help="data-parallel step: 1 = replay it as a captured hipGraph (the all-reduce inside), 0 = launch it eagerly")
    ap.add_argument("--dp-buckets", type=int, default=1 << 20, help="data-parallel step: gradient buckets of at least this many bytes, each all-reduced on a second stream "
                                                                     "while the backward pass of the layers below runs (0: ONE all-reduce of the whole gradient after the backward pass)")
    ap.add_argument("--momentum", type=float, default=0.0, help="SGD momentum (rcn_hipx_set_sgd; 0: plain SGD)")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="SGD weight decay, on every parameter")
    ap.add_argument("--nesterov", action="store_true", help="Nesterov momentum (needs --momentum > 0)")
    ap.add_argument("--optimizer", choices=["sgd", "adam", "adamw"], default="sgd",
                    help="adam / adamw: rcn_hipx_set_adam (torch.optim.Adam's L2 form / torch.optim.AdamW), with --betas, --eps and --weight-decay; not with --momentum / --nesterov")
    ap.add_argument("--betas", type=float, nargs=2, default=(0.9, 0.999), metavar=("B1", "B2"), help="Adam's betas")
    ap.add_argument("--eps", type=float, default=1e-8, help="Adam's eps")
    ap.add_argument("--ema", type=float, default=0.0, metavar="D",
                    help="keep an exponential moving average of the parameters with decay D inside the update launch (rcn_hipx_set_ema; 0: none), set before the "
                         "timed steps; with --dataset the line gains eval_ema_images_per_s and the average's loss / accuracy beside the live ones")
    ap.add_argument("--clip", type=float, default=0.0, metavar="M",
                    help="clip the gradient to a global L2 norm of at most M in front of the update (rcn_hipx_set_clip; 0: off; inf: measure the norm only), set before "
                         "the timed steps: three launches in the step's graph instead of one; the line gains clip_max_norm and grad_norm_last")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="gradient accumulation: every K steps form one update on the mean of their gradients (rcn_hipx_set_accumulate; 1: off), set before the "
                         "warm-up; --warmup and --steps are rounded up to multiples of K; ms_per_step and images/s stay per micro-step, the line gains accumulate "
                         "and ms_per_update (single GPU: the data-parallel step does not accumulate)")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P",
                    help="inverted dropout with rate P behind every dense_relu layer, the masks drawn inside the step's graph (rcn_hipx_set_dropout; 0: off), set "
                         "before the warm-up: a tick launch and two elementwise launches per site in the step's graph; the line gains dropout")
    ap.add_argument("--dropout-seed", type=int, default=0, metavar="S", help="the seed of --dropout's draws; a data-parallel rank draws with S + rank")
    ap.add_argument("--dataset", type=int, default=0, metavar="N",
                    help="also keep a synthetic set of N images resident (uint8 for mnist / cifar, fp32 for synth224), time train_epoch over whole epochs with a fresh "
                         "device permutation each, then evaluate over the set: the line gains epoch_ms_per_step, epoch_images_per_s, eval_images_per_s, graphs_instantiated "
                         "(single GPU only)")
    ap.add_argument("--eval-metrics", action="store_true",
                    help="with --dataset: the evaluation pass once more through evaluate_metrics (top-1 / top-5 counts where the net has 5 classes, confusion matrix): "
                         "the line gains eval_ms, eval_metrics_ms (both per pass over the set) and eval_top5")
    ap.add_argument("--lr-schedule", choices=["none", "warmup_cosine"], default="none",
                    help="with --dataset: time the epochs once more with a per-step rate (warm-up over 5 %% of an epoch, then cosine to 0) from a device tensor: "
                         "recipe_epoch_ms_per_step beside epoch_ms_per_step; graphs_instantiated, after it, shows that no step captured again")
    ap.add_argument("--augment", type=int, default=-1, metavar="PAD",
                    help="with --dataset: those epochs gather through a random crop with PAD zeros of padding and a horizontal flip (k_gather_aug)")
    ap.add_argument("--trap", action="store_true",
                    help="with --dataset: also run one epoch of a warm-up + cosine schedule as one-batch calls with a new FLOAT rate each (a capture per step): "
                         "trap_ms_per_step, trap_graphs_instantiated")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="E",
                    help="with --dataset: time the recipe's epochs once more with the smoothed loss (rcn_hipx_set_loss): mix_epoch_ms_per_step beside recipe_epoch_ms_per_step")
    ap.add_argument("--mix", choices=["none", "mixup", "cutmix", "both"], default="none",
                    help="with --dataset: those epochs mix every batch with its mirror image by mix_plan's records (mixup alpha 0.8, CutMix alpha 1.0; k_gather_mix, pair labels)")
    ap.add_argument("--snapshot-every", type=int, default=0, metavar="N",
                    help="take a full snapshot of the net's state (rcn_hipx_snapshot_dev: ONE pack launch on the net's stream, no synchronise) behind every N-th timed "
                         "step, into one body allocated before the warm-up; the line gains snapshot_sections, snapshot_bytes and snapshot_us, the mean stream time of "
                         "the pack launch from events around it (0: none; single GPU).  With it, --momentum beside --optimizer adam / adamw is allowed: the velocity "
                         "buffer then exists and is carried, so all six sections can be present")
    args = ap.parse_args()
    if (args.label_smoothing != 0.0 or args.mix != "none") and not args.dataset:
        ap.error("--label-smoothing and --mix time the resident epoch: they need --dataset N")
    if args.snapshot_every < 0:
        ap.error("--snapshot-every: N >= 0")
    if args.optimizer != "sgd" and (args.momentum != 0.0 or args.nesterov) and not args.snapshot_every:
        ap.error("--optimizer adam / adamw: --momentum and --nesterov belong to SGD")
    if not 0.0 <= args.ema < 1.0:
        ap.error("--ema: 0 <= D < 1")
    if not args.clip >= 0.0:
        ap.error("--clip: M >= 0 (inf allowed)")
    if not 1 <= args.accumulate <= 65536:
        ap.error("--accumulate: 1 <= K <= 65536")
    if not 0.0 <= args.dropout < 1.0:
        ap.error("--dropout: 0 <= P < 1")
    if not 0.0 <= args.label_smoothing < 1.0:
        ap.error("--label-smoothing: 0 <= E < 1")
    if (args.lr_schedule != "none" or args.augment >= 0 or args.trap) and not args.dataset:
        ap.error("--lr-schedule, --augment and --trap time the resident epoch: they need --dataset N")
    if args.eval_metrics and not args.dataset:
        ap.error("--eval-metrics times the evaluation of the resident set: it needs --dataset N")
    from mercer_research_amd.launch import spawn_ranks, under_launcher
    if args.gpus > 1 and not under_launcher():
        # `python bench_convnet.py --gpus N`: the parent makes no GPU call; it starts N fresh ranks and relays rank 0's line
        sys.exit(spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus, timeout_s=1500.0))
    import torch
    import torch.distributed as dist
    from mercer_research_amd.convnet import ConvNet
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    real_stdout = None
    dp = world > 1 or args.force_dp
    if dp and args.dataset:
        sys.exit("--dataset times the single-GPU epoch; a data-parallel epoch does not exist")
    if dp and args.snapshot_every:
        sys.exit("--snapshot-every times the single-GPU step")
    if dp and args.accumulate > 1:
        sys.exit("--accumulate: the data-parallel step (gradients -> all-reduce -> apply) does not accumulate; accumulation across ranks does not exist")
    K = args.accumulate
    args.steps = -(-args.steps // K) * K                   # whole cycles: the timed steps end on an update
    if dp:
        sys.stdout.flush()
        real_stdout = os.dup(1)                # RCCL's version banner goes to stdout: keep rank 0's stdout to the one JSON line
        os.dup2(2, 1)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    in_shape, layers, B = CONFIGS[args.config]
    B = args.batch or B                                    # per GPU (weak scaling)
    net = ConvNet(in_shape, layers, B, device=local_rank)
    net.init_params(1)                                     # same seed on every rank: identical replicas
    for kv in args.set:
        net.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    net.set_precision(args.precision)
    sgd = args.momentum != 0.0 or args.weight_decay != 0.0 or args.nesterov
    if args.optimizer != "sgd":
        if sgd and args.snapshot_every:
            net.set_sgd(args.momentum, args.weight_decay, args.nesterov)      # (the velocity exists under Adam: a sixth section to carry)
        net.set_adam(tuple(args.betas), args.eps, args.weight_decay, args.optimizer == "adamw")
    elif sgd:
        net.set_sgd(args.momentum, args.weight_decay, args.nesterov)
    if args.ema > 0:
        net.set_ema(args.ema)
    if args.clip > 0:
        net.set_clip(args.clip)
    if K > 1:
        net.set_accumulate(K)
    if args.dropout > 0:
        net.set_dropout(args.dropout, args.dropout_seed + rank)      # (another seed per rank: the same one would drop the same units in every shard)
    rng = np.random.default_rng(rank)
    nbuf = 8 if args.config != "synth224" else 2           # rotate over several resident batches
    xs = [net.to_device(rng.standard_normal((B,) + in_shape).astype(np.float32)) for _ in range(nbuf)]
    ys = [net.to_device(rng.integers(0, 10, B).astype(np.int32)) for _ in range(nbuf)]
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    lr = 1e-3 if args.optimizer != "sgd" and args.config != "synth224" else 0.01 if args.config != "synth224" else 1e-6     # the un-normalised 8-conv stack on noise diverges at larger steps (speed does not depend on it)
    dp_graphs = {}
    dp_mode = None
    if dp:
        # one process per GPU: shard gradients of the mean loss -> ONE all-reduce (RCCL over xGMI) of the flat padded
        # gradient buffer -> identical update on every rank with lr / world (mean over the global batch)
        grad = torch.empty(net.n_padded, dtype=torch.float32, device=net.device)
        comm = torch.cuda.Stream(device=net.device)            # the buckets' all-reduces: beside the backward pass of the layers below them
        n_buckets = [0]

        def dp_body(x, y):
            """gradients -> all-reduce -> apply, enqueued on net.stream (+ the buckets' collectives on `comm`); captured or eager alike"""
            if args.dp_buckets <= 0:
                net.gradients(x, y, grad, loss)
                dist.all_reduce(grad, op=dist.ReduceOp.SUM)
            else:
                # bucket by layer, overlap with the weight gradients of earlier layers.  A bucket's slice of the flat
                # gradient is final once its launches have run (rcn_hipx_gradients_bucket_dev): `comm` waits for exactly that point of
                # net.stream and reduces the slice while net.stream goes on with the layers below; net.stream joins `comm` before the update.
                def on_bucket(piece, k, n):
                    n_buckets[0] = n
                    comm.wait_stream(net.stream)
                    with torch.cuda.stream(comm):
                        dist.all_reduce(piece, op=dist.ReduceOp.SUM)
                net.gradients_bucketed(x, y, grad, loss, args.dp_buckets, on_bucket)
                net.stream.wait_stream(comm)
            if sgd or args.optimizer != "sgd" or args.ema > 0 or args.clip > 0:       # (apply_sgd keeps the average and clips; apply is the plain axpy and does neither)
                net.apply_sgd(grad, 1.0 / world, lr)
            else:
                net.apply(grad, lr / world)

        def eager_step(i):
            with torch.cuda.stream(net.stream):
                dp_body(xs[i % nbuf], ys[i % nbuf])

        def step(i):
            g = dp_graphs.get(i % nbuf)
            if g is None:
                eager_step(i)
            else:
                g.replay()

        dp_mode = "eager"
        for i in range(2 * nbuf):                          # (in either form, so that both take the same number of steps)
            eager_step(i)
        net.synchronize()
        if args.dp_graph:
            # The ~40 launches of the step and the collective between them as ONE captured graph per batch buffer (the single-GPU step
            # has always been one; eagerly the host issues every launch of every step).  The two eager steps per buffer above come first: scratch
            # buffers reach their sizes and RCCL builds its channels outside the capture.  All ranks capture or none does.
            try:
                for b in range(nbuf):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=net.stream):
                        dp_body(xs[b], ys[b])
                    dp_graphs[b] = g
                ok = torch.ones(1, device=net.device)
            except Exception as ex:                        # capture of the collective not supported here: the eager step stands
                sys.stderr.write(f"[bench_convnet] data-parallel step not captured ({ex}); running it eagerly\n")
                dp_graphs.clear()
                ok = torch.zeros(1, device=net.device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if ok.item() == 0:
                dp_graphs.clear()
            dp_mode = "hipGraph" if dp_graphs else "eager"
    else:
        def buffer_of(i):
            """The batch of step i.  A captured step is keyed by its tensors and its kind of micro-step, eight keys at the most: where K does
            not divide the number of buffers, each position in the cycle has one fixed buffer (the late positions share one)."""
            return i % nbuf if nbuf % K == 0 else min(i % K, max(nbuf - 2, 0))

        def step(i):
            net.train_step(xs[buffer_of(i)], ys[buffer_of(i)], lr, loss)
    snap_body, snap_events, snap_last = None, [], None
    if args.snapshot_every:
        snap_last = net.snapshot()                         # (sizes the body; every timed snapshot packs into this one buffer)
        snap_body = snap_last.body
    net.synchronize()
    for i in range(-(-max(args.warmup, 2 * nbuf) // K) * K):      # first use of each (x, y) pair instantiates its graph; whole cycles
        step(i)
    net.synchronize()
    if dp:
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
        if args.snapshot_every and (i + 1) % args.snapshot_every == 0:
            with torch.cuda.stream(net.stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                snap_last = net.snapshot(body=snap_body)
                e1.record()
            snap_events.append((e0, e1))
    net.synchronize()
    if dp:
        dist.barrier()
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if dp:
        t = torch.tensor([el], dtype=torch.float64, device=net.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    flops = net.step_flops(B)
    tf = flops * args.steps / el / 1e12                    # per GPU
    extra = resident_set_figures(net, args, in_shape, B, lr) if args.dataset else {}
    if args.snapshot_every:
        from mercer_research_amd.convnet import SECTIONS
        extra.update({"snapshot_every": args.snapshot_every, "snapshots": len(snap_events),
                      "snapshot_sections": [name for name, bit in SECTIONS.items() if snap_last.desc.sections & bit], "snapshot_bytes": int(snap_last.desc.body_bytes),
                      "snapshot_us": round(sum(a.elapsed_time(b) for a, b in snap_events) / len(snap_events) * 1e3, 2) if snap_events else None})
    if rank == 0:
        # the peak a fraction is quoted against is the peak of the MFMA the GEMMs actually issue: fp32 MFMA (157.3 TF) in fp32
        # mode, dense bf16 MFMA (~2.5 PF) in bf16 mode -- and for the bf16 path, which is HBM-bound, the step's HBM floor
        # (every activation and activation gradient written once and read once per pass, as stored) is the more telling roof
        bf16 = args.precision != "fp32"
        peak = BF16_MFMA_PEAK_TFLOPS if bf16 else F32_MFMA_PEAK_TFLOPS
        floor_bytes = net.step_hbm_floor_bytes(B, stored16=args.precision == "bf16_stored")
        floor_ms = floor_bytes / (HBM_PEAK_GBS * 1e9) * 1e3 if floor_bytes else None
        out_line = json.dumps({"metric": "training images/sec (Track X, trainable conv net; not the BASELINE metric)", "config": args.config, "batch_per_gpu": B, "n_gpus": world,
                          "scaling": "weak", "value": round(world * B * args.steps / el, 1), "unit": "images/s", "ms_per_step": round(el / args.steps * 1e3, 4),
                          "step_gflop_per_gpu": round(flops / 1e9, 3), "achieved_tflops_per_gpu": round(tf, 2),
                          "mfma_peak_tflops": peak, "mfma_peak_kind": "bf16 dense MFMA" if bf16 else "fp32 MFMA",
                          "frac_of_mfma_peak": round(tf / peak, 4),
                          "hbm_floor_ms": round(floor_ms, 4) if floor_ms else None, "frac_of_hbm_floor": round(floor_ms / (el / args.steps * 1e3), 4) if floor_ms else None,
                          "dtype": "f32" if not bf16 else "bf16 MFMA operands (fwd, dgrad, wgrad), f32 accumulate/update" + (", conv-stage activations and gradients stored as bf16" if args.precision == "bf16_stored" else ""), "data": "synthetic", "final_loss": round(loss.item(), 4),
                          "optimizer": args.optimizer, "ema_decay": args.ema,
                          "accumulate": K, "ms_per_update": round(el / args.steps * 1e3 * K, 4),
                          "dropout": args.dropout,
                          "clip_max_norm": args.clip, "grad_norm_last": round(net.grad_norm()[0], 6) if args.clip > 0 else None,
                          "data_parallel_step": dp_mode,
                          "data_parallel_allreduce": (None if not dp else "one all-reduce of the flat gradient after the backward pass" if args.dp_buckets <= 0 else
                                                      f"{n_buckets[0]} buckets of >= {args.dp_buckets} bytes, each all-reduced on a second stream under the backward pass of the layers below"),
                          **extra}) + "\n"
        if real_stdout is not None:
            os.write(real_stdout, out_line.encode())
        else:
            sys.stdout.write(out_line)
    if dp:
        dp_graphs.clear()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
