"""The MORAN recogniser of the word accuracy (`--rec moran`; reference model/moran/: moran.py, morn.py, asrn_res.py).

`MORAN` is the stock-torch mirror of MORAN(1, 37, 256, 32, 100, BidirDecoder=True) in eval mode (`test=True`): same module tree,
parameter names and state_dict layout (427 keys, 20.34 M parameters), so a reference checkpoint loads unchanged.  It runs on whatever
device its tensors are on (the sampling grid is a buffer): the comparison partner of the native path on the GPU and its timing
baseline.  Pinned to the imported reference by tests/golden/moran.npz.  Left out: the debug drawing, fracPickup and the training
branch of the attention, MORN's random "skip rectification" branch; the R2L decoder holds its weights and is not evaluated (the
reference's eval reads the L2R output only, super_resolution.py:455-459).

`NativeMORAN` is the same module tree with all its arithmetic in libdpmn_hip.so (eval mode only):
  prep     dpmn_gray_prep_f32: parse_moran_data (bicubic 32 x 100 + luma, no normalisation) as the plane the warp samples and as
           the NHWC(4) input of the first convs, one launch
  rectify  MORN: per pass dpmn_maxpool2d_f32 x 3 and five NHWC convs (BatchNorm folded, ReLU epilogue) down to the 1 x 4 x 12 offset
           map, then ONE dpmn_moran_rectify_f32 (signed (2, 1) max-pool, bilinear up-sampling, accumulation, zero-padded warp);
           two passes (enhance = 1)
  resnet   ASRN ResNet: conv1 + downsample of a stage's first block are ONE conv with concatenated output channels (stride 2 in
           the descriptor for block1 / block2, stride 1 for the (2, 1) stages), dpmn_moran_split_nhwc_f32 gathers the rows / columns
           and separates the two halves; 1 x 1 conv1 of the later blocks on the pointwise path; ReLU after the residual add in the
           epilogue of conv2
  encode   per BidirectionalLSTM: one GEMM for the input projection of every step and both directions, dpmn_bilstm_f32, the
           embedding Linear on the GEMM path
  decode   i2h(feats) once per batch on the GEMM path, then dpmn_moran_decode_f32: all 20 greedy steps of the L2R attention
           decoder in ONE launch (csrc/moran.hip), ONE device-to-host copy of the ids."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils.labelmaps import MORAN_ALPHABET, moran_strings
from . import packing
from .native import PackedEval, bilstm_stack

MAX_ITER = 20                      # parse_moran_data (base.py:405): every image is decoded for 20 steps
STAGES = ((32, 2, 3), (64, 2, 4), (128, (2, 1), 6), (256, (2, 1), 6), (512, (2, 1), 3))       # asrn_res.py:192-196


class MORN(nn.Module):
    def __init__(self, nc, targetH, targetW):
        super().__init__()
        self.targetH, self.targetW = targetH, targetW
        cbr = lambda i, o: [nn.Conv2d(i, o, 3, 1, 1), nn.BatchNorm2d(o), nn.ReLU(True)]
        self.cnn = nn.Sequential(nn.MaxPool2d(2, 2), *cbr(nc, 64), nn.MaxPool2d(2, 2), *cbr(64, 128), nn.MaxPool2d(2, 2), *cbr(128, 64),
                                 *cbr(64, 16), nn.Conv2d(16, 1, 3, 1, 1), nn.BatchNorm2d(1))
        self.pool = nn.MaxPool2d(2, 1)
        ys = np.arange(targetH) * 2. / (targetH - 1) - 1
        xs = np.arange(targetW) * 2. / (targetW - 1) - 1
        gx, gy = np.meshgrid(xs, ys)
        self.register_buffer("grid", torch.from_numpy(np.stack([gx, gy], -1)[None]).float(), persistent=False)      # (1, H, W, 2): x, y

    def offsets(self, x):
        o = self.cnn(x)
        pooled = self.pool(F.relu(o)) - self.pool(F.relu(-o))
        return F.grid_sample(pooled, self.grid.expand(x.shape[0], -1, -1, -1), mode='bilinear', padding_mode='zeros',
                             align_corners=False).permute(0, 2, 3, 1)

    def warp(self, x, acc):
        grid = self.grid.expand(x.shape[0], -1, -1, -1)
        return F.grid_sample(x, torch.cat([grid[..., 0:1], grid[..., 1:2] + acc], 3), mode='bilinear', padding_mode='zeros', align_corners=False)

    def stages(self, x, enhance=1):
        """-> ([accumulated offsets (B, H, W) after every pass], rectified image); morn.py:48-82 with test=True."""
        x_small = F.interpolate(x, size=(self.targetH, self.targetW), mode='bilinear', align_corners=False)
        acc = self.offsets(x_small)
        accs = [acc[..., 0]]
        rect = self.warp(x, acc)
        for _ in range(enhance):
            acc = acc + self.offsets(rect)
            accs.append(acc[..., 0])
            rect = self.warp(x, acc)
        return accs, rect

    def forward(self, x, test=True, enhance=1, debug=False):
        return self.stages(x, enhance)[1]


class BidirectionalLSTM(nn.Module):
    def __init__(self, nIn, nHidden, nOut):
        super().__init__()
        self.rnn = nn.LSTM(nIn, nHidden, bidirectional=True)
        self.embedding = nn.Linear(nHidden * 2, nOut)

    def forward(self, x):
        rec, _ = self.rnn(x)
        T, b, h = rec.shape
        return self.embedding(rec.reshape(T * b, h)).view(T, b, -1)


class AttentionCell(nn.Module):
    def __init__(self, input_size, hidden_size, num_embeddings=128):
        super().__init__()
        self.i2h = nn.Linear(input_size, hidden_size, bias=False)
        self.h2h = nn.Linear(hidden_size, hidden_size)
        self.score = nn.Linear(hidden_size, 1, bias=False)
        self.rnn = nn.GRUCell(input_size + num_embeddings, hidden_size)
        self.hidden_size, self.input_size, self.num_embeddings = hidden_size, input_size, num_embeddings

    def forward(self, prev_hidden, feats, feats_proj, cur_embeddings):
        """feats (T, B, C), feats_proj = i2h(feats) (T, B, hidden) -> (new hidden, alpha (T, B)); asrn_res.py:39-65 with test=True."""
        emition = self.score(torch.tanh(feats_proj + self.h2h(prev_hidden).unsqueeze(0))).squeeze(2)
        alpha = F.softmax(emition, 0)
        context = (feats * alpha.unsqueeze(2)).sum(0)
        return self.rnn(torch.cat([context, cur_embeddings], 1), prev_hidden), alpha


class Attention(nn.Module):
    def __init__(self, input_size, hidden_size, num_classes, num_embeddings=128):
        super().__init__()
        self.attention_cell = AttentionCell(input_size, hidden_size, num_embeddings)
        self.input_size, self.hidden_size, self.num_classes, self.num_embeddings = input_size, hidden_size, num_classes, num_embeddings
        self.generator = nn.Linear(hidden_size, num_classes)
        self.char_embeddings = nn.Parameter(torch.randn(num_classes + 1, num_embeddings))

    def greedy(self, feats, steps):
        """asrn_res.py:127-144: feats (T, B, C) -> logits (B, steps, num_classes); the next embedding index is arg-max + 1."""
        T, B, C = feats.shape
        proj = self.attention_cell.i2h(feats)
        hidden = feats.new_zeros(B, self.hidden_size)
        y = torch.zeros(B, dtype=torch.long, device=feats.device)
        out = []
        for _ in range(steps):
            hidden, _ = self.attention_cell(hidden, feats, proj, self.char_embeddings.index_select(0, y))
            out.append(self.generator(hidden))
            y = out[-1].max(1)[1] + 1
        return torch.stack(out, 1)


class ResidualBlock(nn.Module):
    def __init__(self, c_in, c_out, stride):
        super().__init__()
        strided = (stride[0] if isinstance(stride, tuple) else stride) > 1
        cb = lambda k, s, p: nn.Sequential(nn.Conv2d(c_in, c_out, k, s, p), nn.BatchNorm2d(c_out, momentum=0.01))
        self.downsample = cb(3, stride, 1) if strided else None
        self.conv1 = cb(3, stride, 1) if strided else cb(1, stride, 0)
        self.conv2 = nn.Sequential(nn.Conv2d(c_out, c_out, 3, 1, 1), nn.BatchNorm2d(c_out, momentum=0.01))
        self.relu = nn.ReLU()

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return self.relu((x if self.downsample is None else self.downsample(x)) + out)


class ResNet(nn.Module):
    def __init__(self, c_in):
        super().__init__()
        self.block0 = nn.Sequential(nn.Conv2d(c_in, 32, 3, 1, 1), nn.BatchNorm2d(32, momentum=0.01))
        cin = 32
        for i, (cout, stride, repeat) in enumerate(STAGES):
            blocks = [ResidualBlock(cin, cout, stride)] + [ResidualBlock(cout, cout, 1) for _ in range(repeat - 1)]
            setattr(self, "block%d" % (i + 1), nn.Sequential(*blocks))
            cin = cout

    def forward(self, x):
        for i in range(6):
            x = getattr(self, "block%d" % i)(x)
        return x


class ASRN(nn.Module):
    def __init__(self, imgH, nc, nclass, nh, BidirDecoder=False):
        super().__init__()
        assert imgH % 16 == 0, 'imgH must be a multiple of 16'
        self.cnn = ResNet(nc)
        self.rnn = nn.Sequential(BidirectionalLSTM(512, nh, nh), BidirectionalLSTM(nh, nh, nh))
        self.BidirDecoder = BidirDecoder
        if BidirDecoder:
            self.attentionL2R = Attention(nh, nh, nclass, 256)
            self.attentionR2L = Attention(nh, nh, nclass, 256)
        else:
            self.attention = Attention(nh, nh, nclass, 256)

    @property
    def l2r(self):
        return self.attentionL2R if self.BidirDecoder else self.attention

    def features(self, x):
        """rectified image -> (ResNet output (B, 512, 1, W), BiLSTM output (T, B, nh))."""
        conv = self.cnn(x)
        assert conv.shape[2] == 1, "the height of conv must be 1"
        return conv, self.rnn(conv.squeeze(2).permute(2, 0, 1).contiguous())


class MORAN(nn.Module):
    def __init__(self, nc=1, nclass=37, nh=256, targetH=32, targetW=100, BidirDecoder=True):
        super().__init__()
        self.nc, self.nclass, self.nh, self.targetH, self.targetW = nc, nclass, nh, targetH, targetW
        self.MORN = MORN(nc, targetH, targetW)
        self.ASRN = ASRN(targetH, nc, nclass, nh, BidirDecoder)

    @staticmethod
    def parse_moran_data(imgs):
        """base.py:396-402: bicubic resize to 32 x 100, ITU-R 601 luma; no normalisation."""
        x = F.interpolate(imgs[:, :3].float(), (32, 100), mode='bicubic')
        return 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]

    @torch.no_grad()
    def stages_gray(self, gray, steps=MAX_ITER):
        """Every intermediate of the eval forward on the (B, 1, 32, 100) recogniser input (stock operators), image-major."""
        accs, rect = self.MORN.stages(gray)
        conv, rnn = self.ASRN.features(rect)
        att = self.ASRN.l2r
        logits = att.greedy(rnn, steps)
        return {"prep": gray, "offsets1": accs[0], "offsets2": accs[1], "rectified": rect, "resnet": conv,
                "rnn": rnn.permute(1, 0, 2).contiguous(), "i2h": att.attention_cell.i2h(rnn).permute(1, 0, 2).contiguous(),
                "logits": logits, "ids": logits.max(2)[1]}

    def stages(self, images01, steps=MAX_ITER):
        return self.stages_gray(self.parse_moran_data(images01), steps)

    @torch.no_grad()
    def forward(self, x, length, text=None, text_rev=None, test=True, debug=False):
        """The reference's eval call rec(tensor, length, text, text_rev, test=True, debug=...): -> (L2R logits (sum(length),
        nclass) with the rows of an image together, None for the R2L decoder), and a None demo image behind it when debug."""
        if self.training or not test:
            raise RuntimeError("dpmn_amd MORAN: only the eval-mode forward with test=True is built")
        steps = int(length.max())
        logits = self._logits(x, steps)
        rows = torch.cat([logits[b, :int(n)] for b, n in enumerate(length.tolist())], 0)
        return ((rows, None), None) if debug else (rows, None)

    def _logits(self, gray, steps):
        return self.stages_gray(gray, steps)["logits"]

    @torch.no_grad()
    def read(self, images):
        """Recognised strings of (B, >=3, H, W) images in [0, 1]."""
        return moran_strings(self.stages(images)["ids"].cpu().numpy())


class NativeMORAN(PackedEval, MORAN):
    """Drop-in for the reference's MORAN(1, 37, 256, 32, 100, BidirDecoder=True) in eval mode, batched, on libdpmn_hip.so (module
    docstring); the torch layers hold the parameters and are never called."""

    EVAL_ONLY = "dpmn_amd NativeMORAN: only the eval-mode forward is built (BatchNorm folded, greedy decoder)"

    def __init__(self, nc=1, nclass=37, nh=256, targetH=32, targetW=100, BidirDecoder=True):
        if (nc, nclass, nh, targetH, targetW, bool(BidirDecoder)) != (1, 37, 256, 32, 100, True):
            raise NotImplementedError("dpmn_amd NativeMORAN: built for MORAN(1, 37, 256, 32, 100, BidirDecoder=True) (MORAN_init's "
                                      "recogniser), got (%r, %r, %r, %r, %r, BidirDecoder=%r)" % (nc, nclass, nh, targetH, targetW, BidirDecoder))
        super().__init__(nc, nclass, nh, targetH, targetW, BidirDecoder)

    def _build_packs(self, sd):
        fold = lambda p, **kw: packing.pack_conv(sd[p + "0.weight"], sd[p + "0.bias"], packing.bn_tuple(sd, p + "1."), **kw)
        morn = []
        for i, ci in enumerate((1, 5, 9, 12, 15)):
            w = sd["MORN.cnn.%d.weight" % ci]
            morn.append(packing.pack_conv(w, sd["MORN.cnn.%d.bias" % ci], packing.bn_tuple(sd, "MORN.cnn.%d." % (ci + 1)),
                                          cin_pad=4 if i == 0 else None) + (w.shape[0],))
        blocks = []
        for si, (cout, stride, repeat) in enumerate(STAGES):
            for bi in range(repeat):
                p = "ASRN.cnn.block%d.%d." % (si + 1, bi)
                c2 = fold(p + "conv2.")
                if bi == 0:      # conv1 and downsample read the same input with the same geometry: one conv, channels [conv1 | downsample]
                    (w1, b1), (wd, bd) = fold(p + "conv1."), fold(p + "downsample.")
                    blocks.append(((torch.cat([w1, wd], 0).contiguous(), torch.cat([b1, bd], 0).contiguous()), c2, cout, stride))
                else:
                    blocks.append((fold(p + "conv1."), c2, cout, None))
        rnn = [packing.pack_bilstm(sd, "ASRN.rnn.%d.rnn." % li) + (sd["ASRN.rnn.%d.embedding.weight" % li].contiguous(),
                                                                   sd["ASRN.rnn.%d.embedding.bias" % li].contiguous()) for li in range(2)]
        a = "ASRN.attentionL2R."
        w_ih, nh = sd[a + "attention_cell.rnn.weight_ih"], self.nh
        dec = {"h2h_w": sd[a + "attention_cell.h2h.weight"].contiguous(), "h2h_b": sd[a + "attention_cell.h2h.bias"].contiguous(),
               "score_w": sd[a + "attention_cell.score.weight"].reshape(-1).contiguous(),
               "E": ops.linear(sd[a + "char_embeddings"].contiguous(), w_ih[:, nh:].contiguous(), sd[a + "attention_cell.rnn.bias_ih"].contiguous()),
               "wih_ctx": w_ih[:, :nh].contiguous(), "whh": sd[a + "attention_cell.rnn.weight_hh"].contiguous(),
               "bhh": sd[a + "attention_cell.rnn.bias_hh"].contiguous(), "gen_w": sd[a + "generator.weight"].contiguous(),
               "gen_b": sd[a + "generator.bias"].contiguous()}
        return {"morn": morn, "block0": fold("ASRN.cnn.block0.", cin_pad=4), "blocks": blocks, "rnn": rnn, "dec": dec,
             "dec_abi": ops.moran_dec_weights(dec), "i2h_w": sd[a + "attention_cell.i2h.weight"].contiguous(),
             "gx": self.MORN.grid[0, 0, :, 0].contiguous(), "gy": self.MORN.grid[0, :, 0, 1].contiguous()}

    # ------------------------------------------------------------------ stages
    # Every stage takes the packs as an optional last argument: the cache key of _packs() walks all ~640 parameters and buffers, so
    # pred_ids() fetches them once per batch and hands them down; called alone (the per-stage parity tests) a stage fetches its own.
    def prep(self, images):
        """(B, >=3, H, W) images in [0, 1] -> (gray plane (B, 1, 32, 100), the same as NHWC (B, 32, 100, 4) with channel 0 = gray)."""
        return ops.moran_prep(images.float(), self.targetH, self.targetW)

    @torch.no_grad()
    def offset_map(self, x_nhwc4, P=None):
        """MORN's offset head: NHWC(4) image -> the (B, 4, 12) offset map."""
        x = x_nhwc4
        for i, (wp, bp, cout) in enumerate((P or self._packs())["morn"]):
            if i < 3:
                x = ops.maxpool2d(x, (2, 2), (2, 2))
            x = ops.conv2d([x], wp, bp, cout, 3, pad=1, epi_act="relu" if i < 4 else "none")
        return x.view(x.shape[0], x.shape[1], x.shape[2])

    @torch.no_grad()
    def rectify(self, plane, x_nhwc4, enhance=1, P=None):
        """-> ([accumulated offsets (B, 32, 100) after every pass], rectified plane (B, 1, 32, 100), rectified NHWC(4))."""
        P = P or self._packs()
        acc, accs, x4 = None, [], x_nhwc4
        for _ in range(1 + enhance):
            acc, rect, x4 = ops.moran_rectify(self.offset_map(x4, P), plane, P["gx"], P["gy"], acc)
            accs.append(acc)
        return accs, rect, x4

    @torch.no_grad()
    def resnet(self, rect_nhwc4, P=None):
        """rectified NHWC(4) image -> ResNet output NHWC (B, 1, 25, 512)."""
        P = P or self._packs()
        wp, bp = P["block0"]
        x = ops.conv2d([rect_nhwc4], wp, bp, 32, 3, pad=1)
        for (w1, b1), (w2, b2), cout, stride in P["blocks"]:
            if stride is None:
                o, res = ops.conv2d([x], w1, b1, cout, 1), x
            elif isinstance(stride, tuple):      # (2, 1): dpmn_conv_desc has one scalar stride -- stride-1 conv, rows gathered by the split
                o, res = ops.moran_split(ops.conv2d([x], w1, b1, 2 * cout, 3, pad=1), stride[0], stride[1])
            else:
                o, res = ops.moran_split(ops.conv2d([x], w1, b1, 2 * cout, 3, stride=stride, pad=1), 1, 1)
            x = ops.conv2d([o], w2, b2, cout, 3, pad=1, epi_act="relu_post_res", res=res)
        return x

    @torch.no_grad()
    def bilstm(self, f, P=None):
        """ResNet output NHWC (B, 1, 25, 512) -> BiLSTM output (B, 25, 256)."""
        x, B, T = self.rows(f)
        return bilstm_stack(x, (P or self._packs())["rnn"], B, T).view(B, T, -1)

    def encode(self, rect_nhwc4, P=None):
        """rectified NHWC(4) image -> BiLSTM output (B, 25, 256)."""
        P = P or self._packs()
        return self.bilstm(self.resnet(rect_nhwc4, P), P)

    def i2h(self, feats, P=None):
        B, T, D = feats.shape
        return ops.linear(feats.reshape(B * T, D), (P or self._packs())["i2h_w"]).view(B, T, -1)

    @torch.no_grad()
    def decode(self, feats, steps=MAX_ITER, P=None):
        """BiLSTM output (B, 25, 256) -> (L2R logits (B, steps, 37), arg-max ids (B, steps) int32), both on the device."""
        self._check_eval()
        P = P or self._packs()
        feats = feats.contiguous()
        return ops.moran_decode(P["dec_abi"], feats, self.i2h(feats, P), steps, self.nclass)

    def _run(self, plane, x4, steps):
        P = self._packs()
        return self.decode(self.encode(self.rectify(plane, x4, 1, P)[2], P), steps, P)

    def _logits(self, gray, steps):
        """the reference's forward on its own input (B, 1, 32, 100)"""
        self._check_eval()
        if tuple(gray.shape[1:]) != (1, self.targetH, self.targetW):
            raise ValueError("dpmn_amd NativeMORAN: forward takes parse_moran_data's (B, 1, 32, 100) tensor")
        plane = gray.contiguous().float()
        return self._run(plane, ops.nchw_to_nhwc(plane, 4), steps)[0]

    @torch.no_grad()
    def pred_ids(self, images):
        """(B, >=3, H, W) images in [0, 1] -> (B, 20) int32 ids on the device."""
        self._check_eval()
        return self._run(*self.prep(images), MAX_ITER)[1]

    @torch.no_grad()
    def read(self, images):
        """Recognised strings of (B, >=3, H, W) images in [0, 1]: every stage on the current stream, then ONE device-to-host copy
        (the arg-max ids) and the cut at '$' on the host."""
        return moran_strings(self.pred_ids(images).cpu().numpy())

    @torch.no_grad()
    def read_conf(self, images):
        """`read` with a confidence (ours; utils/confidence.py) -> (strings, scores, terms): the strings are `read`'s, from the same
        forward pass; score = the sum of the log-softmax values of the arg-max ids up to and with the first '$' (dpmn_attn_conf_f32
        on the decoder's logits), terms = the number of summed steps.  ONE device-to-host copy: the ids with the scores and terms
        behind them."""
        self._check_eval()
        logits, ids = self._run(*self.prep(images), MAX_ITER)
        B, steps = ids.shape
        conf = ops.attn_confidence(logits, ids, MORAN_ALPHABET.index('$'))
        h = torch.cat([ids.reshape(-1), conf]).cpu().numpy()
        n = B * steps
        return (moran_strings(h[:n].reshape(B, steps)), [float(v) for v in h[n:n + B].view("float32")], [int(v) for v in h[n + B:]])

    @torch.no_grad()
    def read_lexicon(self, images, lex):
        """-> (greedy strings, the lexicon's strings, distances): `read`'s strings, then per string the lexicon word at the least
        edit distance (ops.edit_read: the strings packed and uploaded, dpmn_edit_lexicon_i32, one copy back).  An attention decoder
        has no frame posteriors, so lex.mode 'score' is refused."""
        if lex.mode == "score":
            raise ValueError("dpmn_amd NativeMORAN.read_lexicon: the CTC score protocol needs a CTC recogniser (--rec crnn); use mode 'edit'")
        greedy = self.read(images)
        return (greedy,) + ops.edit_read(greedy, lex, images.device)
