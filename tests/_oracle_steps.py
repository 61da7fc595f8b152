"""What tests/test_gpu_convnet_forms.py and tests/test_gpu_convnet_exact.py share: one forward pass, one gradient and two training steps of
a net from a reference's parameters (`run`), and their comparison with the oracle's in the net's precision mode (`check_oracle`).  A
reference is a namespace of spec, flat, x, y and the oracle's logits, loss, grad, params1, params2, loss1 at the step rate LR.  Not a test
file and not a conftest: every assert carries its message."""
import numpy as np
from _convnet_util import close, close_per_tensor

# precision -> (the oracle's mode, tolerance, tolerance after two steps)
MODES = {"fp32": ({}, 2e-4, 4e-4), "bf16": (dict(operand="bf16"), 5e-3, 2e-2), "bf16_stored": (dict(operand="bf16", stored=True), 5e-3, 2e-2)}
# The step rate: small enough that the first step lowers the oracle's loss on every net here.  These nets put the logits layer straight
# on thousands of He-scaled features; at 0.05 the first step overshoots into a saturated softmax (oracle losses of 40 to 190, and inf on
# one net), where the second step compares nothing but the overshoot.
LR = 0.0005
KEYS = ("logits", "loss", "grad", "params1", "loss1", "params2", "loss2")


def run(net, ref, xd, yd):
    """from the reference's parameters: logits, loss and the whole padded gradient, then two training steps (the first eager, the second a
    replayed graph: set_option and a new net both start without cached graphs) with the parameters and the loss after each"""
    import torch
    net.set_params(ref.flat)
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        g = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    out = {"logits": logits.cpu().numpy(), "loss": loss.cpu().numpy(), "grad": g.cpu().numpy(), "grad_logical": net.unpad(g)}
    for k in (1, 2):
        with torch.cuda.stream(net.stream):
            net.train_step(xd, yd, LR, loss)
        net.synchronize()
        out[f"params{k}"], out[f"loss{k}"] = net.get_params(), loss.cpu().numpy()     # loss{k}: the loss BEFORE update k
    return out


def close_loss(tag, got, want, rtol):
    print(f"{tag}: |d| =", abs(float(got) - want), "of", want, "rtol =", rtol)
    assert abs(float(got) - want) <= rtol * max(1.0, want), (tag, float(got), want)


def check_oracle(out, ref, precision):
    """gradients and the parameters after one step: every layer's weights and every layer's biases at that tensor's own scale"""
    _, rtol, rtol2 = MODES[precision]
    in_shape, layers, _ = ref.spec
    close(out["logits"], ref.logits, rtol)
    close_loss("loss", out["loss"][0], ref.loss, rtol)
    close_per_tensor(out["grad_logical"], ref.grad, in_shape, layers, rtol)
    close_loss("loss before the first update", out["loss1"][0], ref.loss, rtol)
    close_per_tensor(out["params1"], ref.params1, in_shape, layers, rtol)
    close(out["params2"], ref.params2, rtol2)
    # ... and the first step's displacement by the same rule: at this step rate it is a few thousandths of the parameters' scale, less
    # than the bf16 tolerance of the parameters themselves.  It is -LR times a gradient held at rtol, plus half an ulp of a parameter (6e-8
    # of scale, inside the rule's 1e-6).  The second step has no such rule below rtol2: measured on the device (eager and replayed agree
    # bit for bit), the gradient at the parameters after one step sits 1e-3 to 2e-2 of a layer's scale from the oracle's AT THE SAME
    # parameters in the bf16 modes (fp32: 1e-6) -- one operand that rounds the other way leaves everything behind it 1e-4 apart, where
    # further operands round the other way a thousand times as often.  rtol2 of the parameters' scale is the project's allowance for it.
    close(out["params1"] - ref.flat.astype(np.float64), ref.params1 - ref.flat, rtol)
    close_loss("loss before the second update", out["loss2"][0], ref.loss1, rtol2)
