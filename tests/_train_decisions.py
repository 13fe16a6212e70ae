"""The device forward's non-smooth choices, for the mask-matched float64
oracle (oracle/train_oracle.Decisions): shared by tests/test_gpu_train.py and
tests/test_gpu_train_fullsize.py."""


def device_decisions(tr, cfg):
    """The non-smooth choices the DEVICE's forward took (ReLU masks, segment-
    max winners), read from the activations the Python-driven step keeps for
    its backward (the state in `Trainer._saved`: train_step's stage records),
    in oracle/train_oracle.Decisions order."""
    from pointgnn_amd.train_step import ComposedStep, GnnStage, PoolStage
    out = []
    fc = tr.fc
    eng, state = tr._saved
    assert isinstance(eng, ComposedStep)

    def relu_masks(names, acts, skip_last):
        n = len(names) - (1 if skip_last else 0)
        for i in range(n):
            w = fc[names[i]].n_out
            out.append((acts[i + 1][:, :w] > 0).cpu().numpy())

    def winners(rows, dst, agg, width):
        idx = dst.long()
        out.append((rows[:, :width] == agg[idx][:, :width]).cpu().numpy())

    for s in state:
        if isinstance(s, PoolStage):
            relu_masks(s.names, s.acts, False)
            winners(s.acts[-1], s.dst, s.agg, fc[s.names[-1]].n_out)
            relu_masks(s.onames, s.oacts, False)
        elif isinstance(s, GnnStage):
            if s.off_names is not None:
                relu_masks(s.off_names, s.off_acts, True)
            for i, n in enumerate(s.enames):    # eacts[0] = ReLU(P - Q)
                out.append((s.eacts[i][:, :fc[n].n_out] > 0).cpu().numpy())
            winners(s.eacts[-1], s.dst, s.agg, fc[s.enames[-1]].n_out)
            relu_masks(s.unames, s.uacts, True)
        else:
            relu_masks(s.cls_names, s.cacts, True)
            for names, a in s.loc:
                relu_masks(names, a, True)
    return out
