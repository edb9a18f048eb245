"""What the native recognisers (NativeCRNN, NativeASTER, NativeMORAN, VisionLAN) share on the host: the cache of the weight
packs, the eval-mode check, the BiLSTM stack behind a conv trunk of height 1, and the frozen state their loaders return."""
from .. import ops


class PackedEval:
    """Mixin in front of the nn.Module mirror whose parameters a native recogniser holds.  The class implements
    `_build_packs(sd)` (detached state dict -> its packs) and names EVAL_ONLY, the text of the train-mode error."""

    EVAL_ONLY = None
    _packed = None

    def _packs(self):
        """The packs, rebuilt when a parameter or buffer moves or changes.  The key walks every tensor of the module: a caller
        with several stages (`read`) fetches the packs once and hands them down as the stages' last argument `P`."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + tuple((b.data_ptr(), b._version) for b in self.buffers())
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        P = self._build_packs({k: v.detach() for k, v in self.state_dict().items()})
        self._packed = (key, P)
        return P

    def _check_eval(self):
        if self.training:
            raise RuntimeError(self.EVAL_ONLY)

    def rows(self, f):
        """conv features NHWC (B, 1, T, C) -> (rows (B*T, C) with row b*T + t, B, T)."""
        if f.shape[1] != 1:
            raise RuntimeError("dpmn_amd %s: the height of the conv features must be 1 (input height 32)" % type(self).__name__)
        B, T = f.shape[0], f.shape[2]
        return f.reshape(B * T, f.shape[3]), B, T


def frozen(model):
    """A loaded recogniser as every loader returns it: no parameter takes a gradient, eval mode."""
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


def bilstm_stack(x, layers, B, T):
    """x (B*T, In) through bidirectional LSTM layers packed by packing.pack_bilstm, each (w_ih, b, w_hh) or, with the embedding
    Linear of a BidirectionalLSTM behind it, (w_ih, b, w_hh, ew, eb): per layer one GEMM for the input projection of every step
    and both directions, the recurrence in dpmn_bilstm_f32, the embedding on the GEMM path."""
    for w_ih, b, w_hh, *emb in layers:
        x = ops.bilstm(ops.linear(x, w_ih, b), w_hh, B, T)
        if emb:
            x = ops.linear(x, *emb)
    return x
