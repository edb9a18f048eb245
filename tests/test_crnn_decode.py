"""Greedy CTC decoding of the CRNN recogniser (--rec crnn) on the host side, against the reference's own strLabelConverter.decode
(tests/golden/crnn_ctc.npz, tools/gen_golden.py gen_crnn_ctc): the class -> character map of model/crnn.py and a restatement of
the collapse rule that the device kernel (dpmn_ctc_greedy_i32) implements.  Plus the TextBase entry points of base.py:411-425.
No GPU needed."""
import inspect

import numpy as np

from helpers import load_golden


def _collapse(row):
    """k_ctc_greedy's rule: keep class c at step t when c != 0 and c differs from the class at step t - 1."""
    out, prev = [], -1
    for c in row:
        if c != 0 and c != prev:
            out.append(int(c))
        prev = c
    return out


def test_alphabet_is_the_reference_converters():
    from dpmn_amd.model.crnn import ALPHABET
    from dpmn_amd.model.visionlan import DICT36
    g = load_golden("crnn_ctc")
    assert ALPHABET == str(g["alphabet"])
    assert ALPHABET != DICT36          # digits first: not VisionLAN's table


def test_collapse_and_class_map_match_reference_decode():
    from dpmn_amd.model.crnn import decode_classes
    g = load_golden("crnn_ctc")
    cls, texts = g["classes"], [str(s) for s in g["texts"]]
    T = cls.shape[1]
    collapsed = [_collapse(r) for r in cls]
    padded = np.zeros_like(cls)
    for i, c in enumerate(collapsed):
        padded[i, :len(c)] = c
    lengths = [len(c) for c in collapsed]
    assert decode_classes(padded, lengths) == texts
    assert "" in texts and any(len(s) == T for s in texts)      # the fixture covers the empty and the full-length string


def test_textbase_has_reference_crnn_entry_points():
    from dpmn_amd.interfaces.base import TextBase
    for name, params in (("CRNN_init", ["self", "path"]), ("parse_crnn_data", ["self", "imgs_input"])):
        fn = getattr(TextBase, name)
        sig = inspect.signature(fn)
        assert list(sig.parameters) == params, "%s%s differs from the reference (base.py:411-425)" % (name, sig)
    assert inspect.signature(TextBase.CRNN_init).parameters["path"].default is None


def test_native_crnn_keeps_the_reference_state_dict_layout():
    from dpmn_amd.model.crnn import CRNN, NativeCRNN
    g = load_golden("crnn")
    m = NativeCRNN(32, 1, 37, 256)
    assert [str(r) for r in g["manifest"]] == ["%s|%s|%s" % (k, ",".join(map(str, v.shape)), str(v.dtype).replace("torch.", ""))
                                               for k, v in m.state_dict().items()]
    assert list(m.state_dict()) == list(CRNN(32, 1, 37, 256).state_dict())
