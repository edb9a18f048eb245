"""Host side of the ASTER recogniser's text handling: the vocabulary (reference utils/labelmaps.py get_vocabulary), `AsterInfo`
(interfaces/base.py:480-492), the prediction half of get_str_list (utils/metrics.py:15-68) and the backtracking of the beam search
(model/recognizer/attention_recognition_head.py:124-184) in numpy on the stored per-step tensors."""
import string

import numpy as np

VOC_TYPES = ('digit', 'lower', 'upper', 'all')


def get_vocabulary(voc_type, EOS='EOS', PADDING='PADDING', UNKNOWN='UNKNOWN'):
    chars = {'digit': string.digits, 'lower': string.digits + string.ascii_lowercase, 'upper': string.digits + string.ascii_letters,
             'all': string.digits + string.ascii_letters + string.punctuation}
    if voc_type not in chars:
        raise KeyError('voc_type Error')
    return list(chars[voc_type]) + [EOS, PADDING, UNKNOWN]


class AsterInfo(object):
    def __init__(self, voc_type):
        assert voc_type in VOC_TYPES
        self.voc_type = voc_type
        self.EOS, self.PADDING, self.UNKNOWN = 'EOS', 'PADDING', 'UNKNOWN'
        self.max_len = 100
        self.voc = get_vocabulary(voc_type, EOS=self.EOS, PADDING=self.PADDING, UNKNOWN=self.UNKNOWN)
        self.char2id = dict(zip(self.voc, range(len(self.voc))))
        self.id2char = dict(zip(range(len(self.voc)), self.voc))
        self.rec_num_classes = len(self.voc)


_KEEP = set(string.digits + string.ascii_letters)


def normalize_text(chars):
    """_normalize_text: digits and ASCII letters only, lower-cased."""
    return ''.join(c for c in chars if c in _KEEP).lower()


def ids_to_strings(pred_rec, info):
    """pred_rec (B, L) class ids -> strings: stop at EOS, skip UNKNOWN, normalise (get_str_list's prediction half)."""
    end, unknown = info.char2id[info.EOS], info.char2id[info.UNKNOWN]
    out = []
    for row in np.asarray(pred_rec):
        chars = []
        for c in row.tolist():
            if c == end:
                break
            if c != unknown:
                chars.append(info.id2char[c])
        out.append(normalize_text(chars))
    return out


def _order_desc(v):
    """indices that sort the rows of v in descending order; equal values keep the lower index first"""
    return np.argsort(-v, axis=1, kind='stable')


def beam_backtrack(symbols, predecessors, scores, batch_size, beam_width, eos):
    """symbols / predecessors (L, B * K) int, scores (L, B * K) float: what the beam search stored at every step -> (B, L) ids of
    the best sequence of every image.  Walks the steps backwards from the last step's beams in score order; a beam that emitted EOS
    at step t replaces the currently worst kept sequence of its image (the k-th EOS found replaces position K - 1 - k mod K), then
    the kept sequences are sorted once more by score."""
    symbols, predecessors, scores = np.asarray(symbols), np.asarray(predecessors), np.asarray(scores)
    L, K, B = symbols.shape[0], beam_width, batch_size
    pos = (np.arange(B) * K)[:, None]
    last = scores[L - 1].reshape(B, K)
    order = _order_desc(last)
    s = np.take_along_axis(last, order, 1).copy()
    found = [0] * B
    back = (order + pos).reshape(-1)
    steps = []
    for t in range(L - 1, -1, -1):
        cur = symbols[t][back].copy()
        back = predecessors[t][back].copy()
        for i in np.nonzero(symbols[t] == eos)[0][::-1].tolist():
            b = i // K
            k = K - (found[b] % K) - 1
            found[b] += 1
            back[b * K + k] = predecessors[t][i]
            cur[b * K + k] = symbols[t][i]
            s[b, k] = scores[t][i]
        steps.append(cur)
    best = (_order_desc(s)[:, 0] + pos[:, 0])
    return np.stack([step[best] for step in reversed(steps)], 1).astype(np.int64)
