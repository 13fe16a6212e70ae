"""The device forward's non-smooth choices, for the mask-matched float64
oracle (oracle/train_oracle.Decisions): shared by tests/test_gpu_train.py and
tests/test_gpu_train_fullsize.py."""


def device_decisions(tr, cfg):
    """The non-smooth choices the DEVICE's forward took (ReLU masks, segment-
    max winners), read from the activations the Python-driven step keeps for
    its backward (`Trainer._saved`), in oracle/train_oracle.Decisions order."""
    out = []
    fc = tr.fc

    def relu_masks(names, acts, skip_last):
        n = len(names) - (1 if skip_last else 0)
        for i in range(n):
            w = fc[names[i]].n_out
            out.append((acts[i + 1][:, :w] > 0).cpu().numpy())

    def winners(rows, dst, agg, width):
        idx = dst.long()
        out.append((rows[:, :width] == agg[idx][:, :width]).cpu().numpy())

    for item in tr._saved:
        if item[0] == 'pool':
            _, names, acts, dst, agg, onames, oacts = item[:7]
            relu_masks(names, acts, False)
            winners(acts[-1], dst, agg, fc[names[-1]].n_out)
            relu_masks(onames, oacts, False)
        elif item[0] == 'gnn':
            (_, enames, hx, xo, e, eacts, dst, agg, unames, uacts, off_names,
             off_acts, c) = item
            if off_names is not None:
                relu_masks(off_names, off_acts, True)
            for i, n in enumerate(enames):      # eacts[0] = ReLU(P - Q)
                out.append((eacts[i][:, :fc[n].n_out] > 0).cpu().numpy())
            winners(eacts[-1], dst, agg, fc[enames[-1]].n_out)
            relu_masks(unames, uacts, True)
        else:
            _, cls_names, cacts, loc = item
            relu_masks(cls_names, cacts, True)
            for names, a in loc:
                relu_masks(names, a, True)
    return out
