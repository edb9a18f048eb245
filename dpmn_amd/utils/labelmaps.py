"""Host side of the ASTER recogniser's text handling: the vocabulary (reference utils/labelmaps.py get_vocabulary), `AsterInfo`
(interfaces/base.py:480-492), the prediction half of get_str_list (utils/metrics.py:15-68) and the backtracking of the beam search
(model/recognizer/attention_recognition_head.py:124-184) in numpy on the stored per-step tensors.  And of the MORAN recogniser's: the
label converter of interfaces/base.py:60-61 (utils/utils_moran.py strLabelConverterForAttention) and the cut at '$'."""
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


# ------------------------------------------------------------------------------------------------ MORAN (reference utils/utils_moran.py)
MORAN_ALPHABET = string.digits + string.ascii_lowercase + '$'      # base.py:60-61: joined with ':' and split again; '$' ends a string


class MoranLabelConverter(object):
    """strLabelConverterForAttention(alphabet, ':') of interfaces/base.py:61: class c <-> MORAN_ALPHABET[c]."""

    def __init__(self, alphabet=MORAN_ALPHABET):
        self.alphabet = list(alphabet)
        self.dict = {c: i for i, c in enumerate(self.alphabet)}

    def encode(self, text):
        """str or list of str -> (LongTensor of the concatenated class ids, LongTensor of the lengths); case is ignored."""
        import torch
        texts = [text] if isinstance(text, str) else list(text)
        return (torch.LongTensor([self.dict[c.lower()] for s in texts for c in s]), torch.LongTensor([len(s) for s in texts]))

    def decode(self, t, length):
        """flat class ids + lengths -> str (one length) or list of str."""
        ids = np.asarray(t).reshape(-1).tolist()
        lens = np.asarray(length).reshape(-1).tolist()
        assert len(ids) == sum(lens), "texts with length: {} does not match declared length: {}".format(len(ids), sum(lens))
        out, i = [], 0
        for n in lens:
            out.append(''.join(self.alphabet[c] for c in ids[i:i + n]))
            i += n
        return out[0] if len(lens) == 1 else out


def moran_strings(ids):
    """(B, L) class ids of the L2R decoder -> strings cut at the first '$' (super_resolution.py:458-459)."""
    conv = MoranLabelConverter()
    ids = np.asarray(ids)
    texts = conv.decode(ids.reshape(-1), [ids.shape[1]] * ids.shape[0])
    return [s.split('$')[0] for s in ([texts] if isinstance(texts, str) else texts)]
