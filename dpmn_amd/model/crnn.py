"""Mirror of the reference's CRNN recogniser (model/crnn/crnn.py:1-79) for ONE job on the SR path: under --arch tatt the trainer
derives TATT's `label_vecs` from the frozen CRNN's logits on the LR image (interfaces/super_resolution.py:165-169, 92-96;
parse_crnn_data base.py:419-425).  It is an input generator of the frozen PSN, not part of the refined hot path, and is built from
stock torch operators (MIOpen convolutions / LSTM on the GPU): same constructor, parameter names and state_dict layout as the
reference class, so `recognizer_best_crnn.pth` loads unchanged.  Pinned to the imported reference by tests/golden/crnn.npz.

`NativeCRNN` is the same module tree with all its arithmetic in libdpmn_hip.so (like model/visionlan.py): the recogniser of the
word accuracy in TextSR.eval / test (`--rec crnn`, TextBase.CRNN_init).  `CRNN` itself stays the stock-operator mirror."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from . import packing
from .native import PackedEval, bilstm_stack, frozen

ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyz"    # strLabelConverter (utils_crnn.py): class c > 0 -> ALPHABET[c - 1], 0 = CTC blank


class BidirectionalLSTM(nn.Module):
    def __init__(self, nIn, nHidden, nOut):
        super().__init__()
        self.rnn = nn.LSTM(nIn, nHidden, bidirectional=True)
        self.embedding = nn.Linear(nHidden * 2, nOut)

    def forward(self, x):
        rec, _ = self.rnn(x)
        T, b, h = rec.shape
        return self.embedding(rec.reshape(T * b, h)).view(T, b, -1)


class CRNN(nn.Module):
    def __init__(self, imgH=32, nc=1, nclass=37, nh=256, n_rnn=2, leakyRelu=False):
        super().__init__()
        assert imgH % 16 == 0, 'imgH has to be a multiple of 16'
        ks, ps, nm = [3, 3, 3, 3, 3, 3, 2], [1, 1, 1, 1, 1, 1, 0], [64, 128, 256, 256, 512, 512, 512]
        cnn = nn.Sequential()

        def conv_relu(i, bn=False):
            cnn.add_module('conv%d' % i, nn.Conv2d(nc if i == 0 else nm[i - 1], nm[i], ks[i], 1, ps[i]))
            if bn:
                cnn.add_module('batchnorm%d' % i, nn.BatchNorm2d(nm[i]))
            cnn.add_module('relu%d' % i, nn.LeakyReLU(0.2, inplace=True) if leakyRelu else nn.ReLU(True))

        conv_relu(0)
        cnn.add_module('pooling0', nn.MaxPool2d(2, 2))
        conv_relu(1)
        cnn.add_module('pooling1', nn.MaxPool2d(2, 2))
        conv_relu(2, True)
        conv_relu(3)
        cnn.add_module('pooling2', nn.MaxPool2d((2, 2), (2, 1), (0, 1)))
        conv_relu(4, True)
        conv_relu(5)
        cnn.add_module('pooling3', nn.MaxPool2d((2, 2), (2, 1), (0, 1)))
        conv_relu(6, True)
        self.cnn = cnn
        self.rnn = nn.Sequential(BidirectionalLSTM(512, nh, nh), BidirectionalLSTM(nh, nh, nclass))

    def forward(self, x):
        conv = self.cnn(x)
        assert conv.shape[2] == 1, "the height of conv must be 1"
        return self.rnn(conv.squeeze(2).permute(2, 0, 1))          # (T = 26, B, nclass)

    @staticmethod
    def parse_crnn_data(imgs):
        """base.py:419-425: bicubic resize to 32x100, ITU-R 601 luma."""
        x = F.interpolate(imgs, (32, 100), mode='bicubic')
        return 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]

    @torch.no_grad()
    def label_vecs(self, images_lr3):
        """super_resolution.py:165-169: softmax over the classes, (T, B, 37) -> (B, 37, 1, T)."""
        logits = self(self.parse_crnn_data(images_lr3.float()))
        return torch.softmax(logits, -1).permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2).contiguous()


def load_crnn(path, device):
    """CRNN_init (base.py:411-417): CRNN(32, 1, 37, 256) + the checkpoint's plain state dict; frozen, eval mode."""
    import os
    if not path or not os.path.isfile(path):
        raise FileNotFoundError("dpmn_amd: --arch tatt on real data needs the frozen CRNN that feeds TATT's label_vecs: "
                                "<resume>/recognizer_best_crnn.pth (super_resolution.py:92) is missing (%r)" % (path,))
    m = CRNN(32, 1, 37, 256).to(device)
    print('loading pretrained crnn model from %s' % path)
    m.load_state_dict(torch.load(path, map_location=device))
    return frozen(m)


def decode_classes(cls, length):
    """Collapsed CTC classes (B, T) + lengths (B), host lists or arrays -> strings (strLabelConverter.decode's alphabet)."""
    return ["".join(ALPHABET[c - 1] for c in row[:n]) for row, n in zip(cls, length)]


class NativeCRNN(PackedEval, CRNN):
    """Drop-in for the reference's CRNN(32, 1, 37, 256) in eval mode, batched, on libdpmn_hip.so: same constructor, module tree and
    state_dict keys as `CRNN` (the torch layers hold the parameters and are never called).
      prep   dpmn_gray_prep_f32: bicubic 32x100 + luma straight into the NHWC(4) layout of the first conv
      cnn    seven NHWC convs (dpmn_conv2d_nhwc_f32) with the eval BatchNorm folded and ReLU in the epilogue; pooling0/1 on
             dpmn_maxpool_f32, pooling2/3 ((2,2), (2,1), (0,1)) on dpmn_maxpool2d_f32
      rnn    per BidirectionalLSTM: one GEMM for the input projection of every step and both directions (b_ih + b_hh folded), the
             recurrence in dpmn_bilstm_f32, the embedding Linear on the GEMM path (37 classes padded to 40 rows)
      decode dpmn_ctc_greedy_i32 (arg-max, collapse, drop blank); dpmn_crnn_label_vecs_f32 for label_vecs.
    Rows stay image-major (b*T + t) from the conv output to the logits; `forward` returns the reference's (T, B, 37) as a view.
    The stages take the packs as an optional last argument (PackedEval._packs)."""

    N_PAD = 40          # the GEMM path writes whole groups of 4 columns
    EVAL_ONLY = "dpmn_amd NativeCRNN: only the eval-mode forward is built (BatchNorm folded)"

    def __init__(self, imgH=32, nc=1, nclass=37, nh=256, n_rnn=2, leakyRelu=False):
        super().__init__(imgH, nc, nclass, nh, n_rnn, leakyRelu)
        if imgH != 32 or nc != 1 or nh != 256 or leakyRelu:
            raise NotImplementedError("dpmn_amd NativeCRNN: built for CRNN(32, 1, nclass, 256) with ReLU (CRNN_init's recogniser)")
        self.nclass = nclass

    def _build_packs(self, sd):
        convs = []
        for i in range(7):
            bn = packing.bn_tuple(sd, "cnn.batchnorm%d." % i) if i in (2, 4, 6) else None
            w = sd["cnn.conv%d.weight" % i]
            wp, bp = packing.pack_conv(w, sd["cnn.conv%d.bias" % i], bn, cin_pad=4 if i == 0 else None)
            convs.append((wp, bp, w.shape[0], w.shape[2], 0 if i == 6 else 1))
        rnn = [packing.pack_bilstm(sd, "rnn.%d.rnn." % li) + packing.pad_rows4(sd["rnn.%d.embedding.weight" % li], sd["rnn.%d.embedding.bias" % li])
               for li in range(2)]
        return {"convs": convs, "rnn": rnn}

    @torch.no_grad()
    def features(self, x_nhwc4, P=None):
        """The conv stack on NHWC input with 4 channels (channel 0 = gray) -> (B, 1, T, 512)."""
        x = x_nhwc4
        for i, (wp, bp, cout, k, pad) in enumerate((P or self._packs())["convs"]):
            x = ops.conv2d([x], wp, bp, cout, k, pad=pad, epi_act="relu")
            if i in (0, 1):
                x = ops.maxpool(x, 2, 2)
            elif i in (3, 5):
                x = ops.maxpool2d(x, (2, 2), (2, 1), (0, 1))
        return x

    @torch.no_grad()
    def logits_rows(self, x_nhwc4, P=None):
        """(B*T, 40) logits, row b*T + t; columns >= nclass are zero padding."""
        P = P or self._packs()
        x, B, T = self.rows(self.features(x_nhwc4, P))
        return bilstm_stack(x, P["rnn"], B, T), B, T

    def forward(self, x_gray):
        """The reference's forward: x_gray (B, 1, 32, W) -> logits (T, B, nclass) (a view of the image-major rows)."""
        self._check_eval()
        x4 = ops.nchw_to_nhwc(x_gray.contiguous().float(), 4)
        rows, B, T = self.logits_rows(x4)
        return rows.view(B, T, -1).permute(1, 0, 2)[..., :self.nclass]

    def prep(self, images):
        """parse_crnn_data on (B, >=3, H, W) images in [0, 1] (channels 0..2 read): NHWC (B, 32, 100, 4), channel 0 = gray."""
        return ops.crnn_prep(images.float(), 32, 100)

    @torch.no_grad()
    def read(self, images):
        """Recognised strings of (B, >=3, H, W) images: prep, CNN, BiLSTMs and greedy CTC decode on the current stream, then ONE
        device-to-host copy of the decoded classes and lengths."""
        self._check_eval()
        rows, B, T = self.logits_rows(self.prep(images), self._packs())
        buf, _, _ = ops.ctc_greedy(rows, B, T, self.nclass)
        h = buf.cpu().numpy()
        return decode_classes(h[:B * T].reshape(B, T), h[B * T:])

    @torch.no_grad()
    def read_lexicon(self, images, lex):
        """Open-vocabulary and lexicon-constrained reading in one forward pass (ours; ops.Lexicon) -> (greedy strings, the lexicon's
        strings, scores).  The greedy strings are `read`'s.  Default / lex.mode 'score': dpmn_ctc_lexicon_f32 on the same logits
        rows picks the word of the highest CTC log-likelihood -- the scores are those log-likelihoods ('' and -inf when no word fits
        the T frames) -- and ONE device-to-host copy brings both results.  lex.mode 'edit': the word nearest to the greedy string
        (ops.edit_read), the scores are the distances."""
        self._check_eval()
        if lex.mode == "edit":
            greedy = self.read(images)
            return (greedy,) + ops.edit_read(greedy, lex, images.device)
        rows, B, T = self.logits_rows(self.prep(images), self._packs())
        buf, _, _ = ops.ctc_greedy(rows, B, T, self.nclass, extra=2 * B)
        ops.ctc_lexicon(rows, B, T, self.nclass, lex, out=buf[B * T + B:])
        h = buf.cpu().numpy()
        n = B * T + B
        greedy = decode_classes(h[:B * T].reshape(B, T), h[B * T:n])
        return greedy, lex.strings(h[n:n + B]), [float(v) for v in h[n + B:].view("float32")]

    @torch.no_grad()
    def read_beam(self, images, lm=None, width=16, alpha=0.5, beta=0.0):
        """Greedy and beam-search reading in one forward pass (ours; utils/beam.py, ops.ctc_beam) -> (greedy strings, the beam
        search's strings, scores).  The greedy strings are `read`'s.  The CTC prefix beam search of `width` prefixes runs on the same
        logits rows in one launch (dpmn_ctc_beam_f64), weighing every new symbol with alpha times the character model lm (an
        ops.CharLM; None: no model) plus beta; the scores (float64) are log P_CTC(prefix) + its model score.  Its result lies
        behind the greedy decode's in the same buffer: ONE device-to-host copy brings both."""
        self._check_eval()
        rows, B, T = self.logits_rows(self.prep(images), self._packs())
        buf, _, _ = ops.ctc_greedy(rows, B, T, self.nclass, extra=B * T + 3 * B)
        ops.ctc_beam(rows, B, T, self.nclass, lm, width, alpha, beta, out=buf[B * T + B:])
        h = buf.cpu().numpy()
        n = B * T + B
        cls, length, scores = ops.ctc_beam_decode(h[n:], B, T)
        return decode_classes(h[:B * T].reshape(B, T), h[B * T:n]), decode_classes(cls, length), [float(v) for v in scores]

    @torch.no_grad()
    def read_conf(self, images):
        """`read` with a confidence (ours; utils/confidence.py) -> (strings, scores, terms): the strings are `read`'s, from the same
        forward pass; score = the CTC log-likelihood of each image's own greedy string (dpmn_ctc_conf_f32 on the same logits rows,
        written behind the lengths so that ONE device-to-host copy brings everything), terms = max(its length, 1).
        utils.confidence.confidence(scores, terms) gives exp(score / terms)."""
        self._check_eval()
        rows, B, T = self.logits_rows(self.prep(images), self._packs())
        buf, _, _ = ops.ctc_greedy(rows, B, T, self.nclass, extra=B)
        ops.ctc_confidence(rows, B, T, self.nclass, buf)
        h = buf.cpu().numpy()
        n = B * T + B
        length = h[B * T:n]
        return (decode_classes(h[:B * T].reshape(B, T), length), [float(v) for v in h[n:n + B].view("float32")],
                [max(int(v), 1) for v in length])

    @torch.no_grad()
    def window_rows(self, images):
        """The frame logits of (B, >=3, H, W) images, the windows of tiled lines -> (rows (B*T, 40), B, T): `read`'s stages up to the
        decode, everything still on the device.  The rows of several calls, concatenated in plan order, are read_lines' input."""
        self._check_eval()
        return self.logits_rows(self.prep(images), self._packs())

    @torch.no_grad()
    def read_lines(self, rows, plan, gap=0, lr_w=64, lexicon=None, penalty=0.0):
        """One read per tiled line (ours; utils/line_read.py): rows = window_rows' logits of the windows of `plan` (utils/tile.py: an
        (image, x0) per window, lr_w columns wide) -> (strings, scores, terms, spans), one entry per image: the windows' frame
        posteriors blended along the line (dpmn_line_stitch_f32), decoded once (dpmn_line_greedy_i32) and scored once
        (dpmn_line_ctc_f32: the CTC log-likelihood of the line's own string, terms = max(its symbols, 1)) -- three launches and ONE
        device-to-host copy.  spans: per symbol the (first, last) line frame of its arg-max run.  gap >= 1: a space goes into the
        string where at least `gap` line frames lie between two symbols' runs (utils.line_read.insert_spaces, a heuristic: the CRNN
        has no space class; scores, terms and spans are those of the symbols).  An image of one window gives `read`'s string.
        lexicon (an ops.Lexicon) [penalty]: the same stitched posteriors are also read as a sequence of the lexicon's words
        (ops.line_words_records; utils/line_words.py), its records behind the scores in the same buffer -- still ONE device-to-host
        copy -- and the tuple gains three items: the words joined by single spaces, the Viterbi scores (float64) and the words'
        (first, last) frame spans.  Without a lexicon the return and the launches are unchanged."""
        from ..utils.line_read import SPACE, insert_spaces
        if not len(plan) or rows.shape[0] % len(plan):
            raise ValueError("dpmn_amd NativeCRNN.read_lines: %d logits rows do not divide into the plan's %d windows" % (rows.shape[0], len(plan)))
        line_lp, lines = ops.line_stitch(rows, rows.shape[0] // len(plan), self.nclass, plan, lr_w)
        B, N = len(lines), lines.frames
        buf = ops.line_greedy(line_lp, lines, extra=B if lexicon is None else 3 * N + 5 * B)[0]
        ops.line_ctc_confidence(line_lp, lines, buf)
        if lexicon is not None:
            ops.line_words_records(line_lp, lines, lexicon, penalty, out=buf[3 * N + 2 * B:])
        h = buf.cpu().numpy()
        length = h[3 * N:3 * N + B]
        strings, spans = [], []
        for (f0, _), n in zip(lines, length.tolist()):
            spans.append(list(zip(h[N + f0:N + f0 + n].tolist(), h[2 * N + f0:2 * N + f0 + n].tolist())))
            strings.append("".join(" " if c == SPACE else ALPHABET[c - 1] for c in insert_spaces(h[f0:f0 + n].tolist(), spans[-1], gap)))
        out = strings, [float(v) for v in h[3 * N + B:3 * N + 2 * B].view("float32")], [max(int(n), 1) for n in length], spans
        if lexicon is None:
            return out
        reads = ops.line_words_decode(h[3 * N + 2 * B:], lines)
        return out + ([" ".join(lexicon.words[w] for w in r[0]) for r in reads], [r[2] for r in reads], [r[1] for r in reads])

    @torch.no_grad()
    def label_vecs(self, images_lr3):
        """super_resolution.py:165-169 on the native path: (B, 37, 1, T) softmax of the logits."""
        self._check_eval()
        rows, B, T = self.logits_rows(self.prep(images_lr3), self._packs())
        return ops.crnn_label_vecs(rows, B, T, self.nclass)
