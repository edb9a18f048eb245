"""The ASTER recogniser of the word accuracy (`--rec aster`, the default; reference model/recognizer/: recognizer_builder.py,
stn_head.py, tps_spatial_transformer.py, resnet_aster.py, attention_recognition_head.py).

`ASTER` is the stock-torch mirror of RecognizerBuilder(arch='ResNet_ASTER', rec_num_classes=97, sDim=512, attDim=512,
max_len_labels=100, eos=94, STN_ON=True): same module tree, parameter names and state_dict layout (384 keys), so
`torch.load(path)['state_dict']` loads unchanged.  It runs on whatever device its tensors are on: the comparison partner of the
native path on the GPU and its timing baseline.  Pinned to the imported reference by tests/golden/aster.npz.

`NativeASTER` is the same module tree with all its arithmetic in libdpmn_hip.so (eval mode only):
  prep     dpmn_aster_prep_f32: x * 2 - 1 as the NCHW image the TPS samples + the bilinear 32 x 64 NHWC(4) input of the STN head
  rectify  STN head: six NHWC convs (BatchNorm folded, ReLU epilogue), five 2 x 2 dpmn_maxpool_f32, dpmn_stn_fc_f32; then
           dpmn_tps_sample_f32 to 32 x 100
  encode   ResNet_ASTER: 45 NHWC convs with the BatchNorm folded and ReLU after the residual add in the epilogue; a strided 1 x 1
           conv is dpmn_subsample_nhwc_f32 (the row / column gather) + a pointwise conv, which also serves the (2, 1) strides; then
           per LSTM layer one GEMM for the input projection of every step and both directions + dpmn_bilstm_f32
  decode   csrc/aster.hip: xEmbed(feats) once per batch on the GEMM path, the beam search in four launches per step without a host
           synchronisation, ONE device-to-host copy of the stored symbols / predecessors / scores, backtracking in numpy
           (utils/labelmaps.py beam_backtrack)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils.labelmaps import AsterInfo, beam_backtrack, ids_to_strings
from . import packing
from .native import PackedEval, bilstm_stack
from .stn import TPSSpatialTransformer

TPS_INPUT, TPS_OUTPUT, N_CTRL, TPS_MARGINS, BEAM = (32, 64), (32, 100), 20, (0.05, 0.05), 5
LAYERS = ((32, 3, (2, 2)), (64, 4, (2, 2)), (128, 6, (2, 1)), (256, 6, (2, 1)), (512, 3, (2, 1)))


def _conv3x3_block(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class RecSTNHead(nn.Module):
    """model/recognizer/stn_head.py: input 32 x 64, five 2 x 2 pools, stn_fc1 on 32 * 64 / 4 = 512 features."""

    def __init__(self, in_planes=3, num_ctrlpoints=N_CTRL):
        super().__init__()
        self.num_ctrlpoints = num_ctrlpoints
        chans = [in_planes, 32, 64, 128, 256, 256, 256]
        mods = []
        for i in range(6):
            mods.append(_conv3x3_block(chans[i], chans[i + 1]))
            if i < 5:
                mods.append(nn.MaxPool2d(2, 2))
        self.stn_convnet = nn.Sequential(*mods)
        self.stn_fc1 = nn.Sequential(nn.Linear(TPS_INPUT[0] * TPS_INPUT[1] // 4, 512), nn.BatchNorm1d(512), nn.ReLU(inplace=True))
        self.stn_fc2 = nn.Linear(512, num_ctrlpoints * 2)

    def forward(self, x):
        x = self.stn_convnet(x)
        feat = self.stn_fc1(x.reshape(x.shape[0], -1))
        return feat, self.stn_fc2(0.1 * feat).view(-1, self.num_ctrlpoints, 2)


class AsterBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=(1, 1), downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNetASTER(nn.Module):
    def __init__(self):
        super().__init__()
        self.layer0 = nn.Sequential(nn.Conv2d(3, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True))
        inplanes = 32
        for li, (planes, blocks, stride) in enumerate(LAYERS):
            down = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
            seq = [AsterBlock(inplanes, planes, stride, down)] + [AsterBlock(planes, planes) for _ in range(1, blocks)]
            setattr(self, "layer%d" % (li + 1), nn.Sequential(*seq))
            inplanes = planes
        self.rnn = nn.LSTM(512, 256, bidirectional=True, num_layers=2, batch_first=True)
        self.out_planes = 512

    def features(self, x):
        """[layer0 .. layer5 outputs]"""
        outs = [self.layer0(x)]
        for li in range(1, 6):
            outs.append(getattr(self, "layer%d" % li)(outs[-1]))
        return outs

    def forward(self, x):
        x5 = self.features(x)[-1]
        return self.rnn(x5.squeeze(2).transpose(2, 1))[0]


class AttentionUnit(nn.Module):
    def __init__(self, sDim, xDim, attDim):
        super().__init__()
        self.sEmbed, self.xEmbed, self.wEmbed = nn.Linear(sDim, attDim), nn.Linear(xDim, attDim), nn.Linear(attDim, 1)

    def forward(self, x, sPrev):
        B, T, _ = x.shape
        xProj = self.xEmbed(x.reshape(B * T, -1)).view(B, T, -1)
        sProj = self.sEmbed(sPrev.squeeze(0)).unsqueeze(1)
        return F.softmax(self.wEmbed(torch.tanh(sProj + xProj).view(B * T, -1)).view(B, T), dim=1)


class DecoderUnit(nn.Module):
    def __init__(self, sDim, xDim, yDim, attDim):
        super().__init__()
        self.attention_unit = AttentionUnit(sDim, xDim, attDim)
        self.tgt_embedding = nn.Embedding(yDim + 1, attDim)       # the last row is <BOS>
        self.gru = nn.GRU(input_size=xDim + attDim, hidden_size=sDim, batch_first=True)
        self.fc = nn.Linear(sDim, yDim)

    def forward(self, x, sPrev, yPrev, need_alpha=False):
        alpha = self.attention_unit(x, sPrev)
        context = torch.bmm(alpha.unsqueeze(1), x).squeeze(1)
        out, state = self.gru(torch.cat([self.tgt_embedding(yPrev.long()), context], 1).unsqueeze(1), sPrev)
        out = self.fc(out.squeeze(1))
        return (out, state, alpha) if need_alpha else (out, state)


class AttentionRecognitionHead(nn.Module):
    def __init__(self, num_classes, in_planes, sDim, attDim, max_len_labels):
        super().__init__()
        self.num_classes, self.sDim, self.max_len_labels = num_classes, sDim, max_len_labels
        self.decoder = DecoderUnit(sDim=sDim, xDim=in_planes, yDim=num_classes, attDim=attDim)

    @torch.no_grad()
    def beam_search(self, x, beam_width, eos, return_stored=False):
        """attention_recognition_head.py:68-184 with stock torch operators in the reference's loop structure (every step: the whole
        decoder on the beam-inflated encoder features, log-softmax, top-k, index_select of the state); the backtracking runs on
        the host on one copy of the stored tensors."""
        B, T, D = x.shape
        K, C, dev = beam_width, self.num_classes, x.device
        feats = x.unsqueeze(1).expand(B, K, T, D).reshape(B * K, T, D).contiguous()
        state = torch.zeros(1, B * K, self.sDim, device=dev)
        pos = (torch.arange(B, device=dev) * K).view(-1, 1)
        seq = torch.full((B * K, 1), -float('inf'), device=dev)
        seq[::K] = 0.0
        y_prev = torch.full((B * K,), C, device=dev, dtype=torch.long)
        sym, pred, score = [], [], []
        for _ in range(self.max_len_labels):
            out, state = self.decoder(feats, state, y_prev)
            cand = (seq + F.log_softmax(out, dim=1)).view(B, -1)
            top, idx = cand.topk(K, dim=1)
            y_prev = (idx % C).view(B * K)
            seq = top.view(B * K, 1)
            p = (idx // C + pos).view(B * K)
            state = state.index_select(1, p)
            score.append(seq.view(-1).clone())
            seq = seq.masked_fill(y_prev.view(-1, 1).eq(eos), -float('inf'))
            pred.append(p)
            sym.append(y_prev)
        stored = torch.stack([torch.stack(sym).float(), torch.stack(pred).float(), torch.stack(score)]).cpu().numpy()
        s, p, sc = stored[0].astype(np.int64), stored[1].astype(np.int64), stored[2]
        rec = torch.from_numpy(beam_backtrack(s, p, sc, B, K, eos))
        if return_stored:
            return rec, {"symbols": s, "predecessors": p, "scores": sc}
        return rec, torch.ones_like(rec)


class ASTER(nn.Module):
    def __init__(self, arch='ResNet_ASTER', rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True):
        super().__init__()
        if arch != 'ResNet_ASTER' or not STN_ON:
            raise NotImplementedError("dpmn_amd ASTER: arch 'ResNet_ASTER' with STN_ON=True (Aster_init's recogniser)")
        self.arch, self.rec_num_classes, self.sDim, self.attDim = arch, rec_num_classes, sDim, attDim
        self.max_len_labels, self.eos, self.STN_ON, self.tps_inputsize = max_len_labels, eos, STN_ON, list(TPS_INPUT)
        self.encoder = ResNetASTER()
        self.decoder = AttentionRecognitionHead(rec_num_classes, self.encoder.out_planes, sDim, attDim, max_len_labels)
        self.tps = TPSSpatialTransformer(output_image_size=TPS_OUTPUT, num_control_points=N_CTRL, margins=TPS_MARGINS)
        self.stn_head = RecSTNHead(3, N_CTRL)

    def tps_torch(self, x, ctrl):
        """TPSSpatialTransformer.forward with stock operators (model/stn.py's module runs it in libdpmn_hip.so)."""
        t = self.tps
        B = x.shape[0]
        Y = torch.cat([ctrl, t.padding_matrix.expand(B, 3, 2)], 1)
        src = torch.matmul(t.target_coordinate_repr, torch.matmul(t.inverse_kernel, Y))
        grid = 2.0 * torch.clamp(src.view(-1, TPS_OUTPUT[0], TPS_OUTPUT[1], 2), 0, 1) - 1.0
        return F.grid_sample(x, grid, align_corners=False)

    @torch.no_grad()
    def stages(self, images01):
        """Every intermediate of the eval forward on (B, >=3, H, W) images in [0, 1] (stock operators)."""
        x = images01[:, :3].float() * 2 - 1
        stn_in = F.interpolate(x, self.tps_inputsize, mode='bilinear', align_corners=True)
        _, ctrl = self.stn_head(stn_in)
        rect = self.tps_torch(x, ctrl)
        layers = self.encoder.features(rect)
        enc = self.encoder.rnn(layers[-1].squeeze(2).transpose(2, 1))[0].contiguous()
        return {"stn_input": stn_in, "ctrl": ctrl, "rectified": rect, "layers": layers, "encoder": enc}

    @torch.no_grad()
    def forward(self, input_dict):
        """Eval forward of RecognizerBuilder: {'images': x in [-1, 1], ...} -> {'output': {'pred_rec', 'pred_rec_score'}}; the
        reference's eval-mode loss_rec (against targets parse_aster_data fills with ones) is not built."""
        if self.training:
            raise RuntimeError("dpmn_amd ASTER: only the eval-mode forward is built")
        rec, ones = self.decoder.beam_search(self.stages((input_dict['images'] + 1) * 0.5)["encoder"], BEAM, self.eos)
        return {'losses': {}, 'output': {'pred_rec': rec, 'pred_rec_score': ones}}

    @torch.no_grad()
    def read(self, images, info=None):
        rec, _ = self.decoder.beam_search(self.stages(images)["encoder"], BEAM, self.eos)
        return ids_to_strings(rec.numpy(), info or AsterInfo('all'))


class NativeASTER(PackedEval, ASTER):
    """Drop-in for the reference's ASTER recogniser in eval mode, batched, on libdpmn_hip.so (module docstring); the torch layers
    hold the parameters and are never called."""

    EVAL_ONLY = "dpmn_amd NativeASTER: only the eval-mode forward is built (BatchNorm folded, beam search)"

    def __init__(self, arch='ResNet_ASTER', rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True):
        super().__init__(arch, rec_num_classes, sDim, attDim, max_len_labels, eos, STN_ON)
        if sDim != 512 or attDim != 512 or max_len_labels != 100 or not (0 <= eos < rec_num_classes <= 128):
            raise NotImplementedError("dpmn_amd NativeASTER: built for sDim = attDim = 512, max_len_labels = 100, up to 128 classes")
        self.info = AsterInfo('all') if rec_num_classes == 97 else None

    def _build_packs(self, sd):
        stn = []
        for i in range(6):
            p = "stn_head.stn_convnet.%d." % (2 * i)
            w = sd[p + "0.weight"]
            stn.append(packing.pack_conv(w, sd[p + "0.bias"], packing.bn_tuple(sd, p + "1."), cin_pad=4 if i == 0 else None) + (w.shape[0],))
        fold = lambda conv, bn, **kw: packing.pack_conv(sd["encoder." + conv + ".weight"], None, packing.bn_tuple(sd, "encoder." + bn + "."), **kw)
        blocks = []
        for li, (planes, n, stride) in enumerate(LAYERS):
            for bi in range(n):
                p = "layer%d.%d." % (li + 1, bi)
                down = fold(p + "downsample.0", p + "downsample.1") if bi == 0 else None
                blocks.append((fold(p + "conv1", p + "bn1"), fold(p + "conv2", p + "bn2"), down, planes, stride if bi == 0 else (1, 1)))
        rnn = [packing.pack_bilstm(sd, "encoder.rnn.", li) for li in range(2)]
        d = "decoder.decoder."
        w_ih, D = sd[d + "gru.weight_ih_l0"], self.attDim
        dec = {"s_w": sd[d + "attention_unit.sEmbed.weight"].contiguous(), "s_b": sd[d + "attention_unit.sEmbed.bias"].contiguous(),
               "w_w": sd[d + "attention_unit.wEmbed.weight"].reshape(-1).contiguous(), "w_b": sd[d + "attention_unit.wEmbed.bias"].contiguous(),
               "E": ops.linear(sd[d + "tgt_embedding.weight"].contiguous(), w_ih[:, :D].contiguous(), sd[d + "gru.bias_ih_l0"].contiguous()),
               "wih_ctx": w_ih[:, D:].contiguous(), "whh": sd[d + "gru.weight_hh_l0"].contiguous(), "bhh": sd[d + "gru.bias_hh_l0"].contiguous(),
               "fc_w": sd[d + "fc.weight"].contiguous(), "fc_b": sd[d + "fc.bias"].contiguous()}
        return {"stn": stn, "fc1_t": sd["stn_head.stn_fc1.0.weight"].t().contiguous(), "layer0": fold("layer0.0", "layer0.1", cin_pad=4),
             "blocks": blocks, "rnn": rnn, "dec": dec, "dec_abi": ops.aster_dec_weights(dec),
             "x_w": sd[d + "attention_unit.xEmbed.weight"].contiguous(), "x_b": sd[d + "attention_unit.xEmbed.bias"].contiguous()}

    # ------------------------------------------------------------------ stages (the packs as an optional last argument: PackedEval._packs)
    def prep(self, images):
        """(B, >=3, H, W) images in [0, 1] -> (normalised NCHW (B, 3, H, W), STN input NHWC (B, 32, 64, 4))."""
        return ops.aster_prep(images.float(), *TPS_INPUT)

    @torch.no_grad()
    def rectify(self, norm, stn_in, P=None):
        """-> (control points (B, 20, 2), rectified image (B, 3, 32, 100))."""
        P = P or self._packs()
        x = stn_in
        for i, (wp, bp, cout) in enumerate(P["stn"]):
            x = ops.conv2d([x], wp, bp, cout, 3, pad=1, epi_act="relu")
            if i < 5:
                x = ops.maxpool(x, 2, 2)
        fc1, bn1, fc2 = self.stn_head.stn_fc1[0], self.stn_head.stn_fc1[1], self.stn_head.stn_fc2
        _, ctrl = ops.stn_fc(x, None, P["fc1_t"], fc1.bias, bn1, False, fc2.weight, fc2.bias)
        ctrl = ctrl.view(-1, N_CTRL, 2)
        rect, _ = ops.tps_sample(norm, ctrl, self.tps.inverse_kernel, self.tps.target_coordinate_repr, TPS_OUTPUT)
        return ctrl, rect

    @torch.no_grad()
    def resnet(self, rect, P=None):
        """rectified NCHW image -> [layer0 .. layer5 outputs], NHWC."""
        P = P or self._packs()
        wp, bp = P["layer0"]
        x = ops.conv2d([ops.nchw_to_nhwc(rect.contiguous(), 4)], wp, bp, 32, 3, pad=1, epi_act="relu")
        outs, bi = [x], 0
        for planes, n, _ in LAYERS:
            for _ in range(n):
                (w1, b1), (w2, b2), down, _, stride = P["blocks"][bi]
                bi += 1
                xin = x if stride == (1, 1) else ops.subsample_nhwc(x, *stride)
                res = x if down is None else ops.conv2d([xin], down[0], down[1], planes, 1)
                o = ops.conv2d([xin], w1, b1, planes, 1, epi_act="relu")
                x = ops.conv2d([o], w2, b2, planes, 3, pad=1, epi_act="relu_post_res", res=res)
            outs.append(x)
        return outs

    @torch.no_grad()
    def encode(self, rect, P=None):
        """rectified image -> encoder features (B, 25, 512)."""
        P = P or self._packs()
        x, B, T = self.rows(self.resnet(rect, P)[-1])
        return bilstm_stack(x, P["rnn"], B, T).view(B, T, -1)

    def xproj(self, feats, P=None):
        P = P or self._packs()
        B, T, D = feats.shape
        return ops.linear(feats.reshape(B * T, D), P["x_w"], P["x_b"]).view(B, T, -1)

    @torch.no_grad()
    def decode_step(self, feats, row_img, state, y_prev, P=None):
        """One teacher-forced decoder step: row r attends to image row_img[r]; state (R, 512), y_prev (R) -> (logits (R, n_class),
        new state, alpha (R, T))."""
        self._check_eval()
        P = P or self._packs()
        i32 = lambda t: t.to(device=feats.device, dtype=torch.int32).contiguous()
        return ops.aster_decode_step(P["dec_abi"], feats.contiguous(), self.xproj(feats, P), i32(row_img), state.contiguous().float(), i32(y_prev),
                                     self.rec_num_classes)

    @torch.no_grad()
    def beam_search(self, feats, beam_width=BEAM, eos=None, return_stored=False, P=None):
        """-> pred_rec (B, 100) int64 on the host (+ the stored symbols / predecessors / scores, (100, B * 5) each)."""
        self._check_eval()
        if beam_width != BEAM:
            raise NotImplementedError("dpmn_amd NativeASTER: beam width 5 (recognizer_builder.py:24)")
        eos = self.eos if eos is None else eos
        P = P or self._packs()
        feats = feats.contiguous()
        B = feats.shape[0]
        buf = ops.aster_beam(P["dec_abi"], feats, self.xproj(feats, P), beam_width, self.rec_num_classes, eos, self.max_len_labels)
        h = buf.cpu().numpy()
        s, p, sc = h[0].astype(np.int64), h[1].astype(np.int64), h[2].view(np.float32)
        rec = torch.from_numpy(beam_backtrack(s, p, sc, B, beam_width, eos))
        if return_stored:
            return rec, {"symbols": s, "predecessors": p, "scores": sc}
        return rec

    @torch.no_grad()
    def pred_rec(self, images):
        self._check_eval()
        P = self._packs()
        return self.beam_search(self.encode(self.rectify(*self.prep(images), P)[1], P), P=P)

    @torch.no_grad()
    def forward(self, input_dict):
        """RecognizerBuilder's eval forward: {'images': (B, 3, H, W) in [-1, 1], 'rec_targets', 'rec_lengths'} ->
        {'losses': {}, 'output': {'pred_rec': (B, 100) int64, 'pred_rec_score': ones}}.  The reference also returns an eval-mode
        loss_rec, computed against the targets parse_aster_data fills with ones; it is not built."""
        rec = self.pred_rec((input_dict['images'].float() + 1) * 0.5).to(input_dict['images'].device)
        return {'losses': {}, 'output': {'pred_rec': rec, 'pred_rec_score': torch.ones_like(rec)}}

    @torch.no_grad()
    def read(self, images, info=None):
        """Recognised strings of (B, >=3, H, W) images in [0, 1]: every stage on the current stream, then ONE device-to-host copy
        (the beam search's stored tensors) and the host backtracking."""
        info = info or self.info
        if info is None:
            raise ValueError("dpmn_amd NativeASTER.read: pass the AsterInfo of this vocabulary")
        return ids_to_strings(self.pred_rec(images).numpy(), info)

    @torch.no_grad()
    def read_conf(self, images, info=None):
        """`read` with a confidence (ours; utils/confidence.py) -> (strings, scores, terms): the strings are `read`'s, from the same
        forward pass; score = the stored sequence score of the returned hypothesis at the step where it ends, terms = its length
        counted with the EOS.  Host code over the stored tensors that `read`'s single copy already brings
        (utils.confidence.beam_score): no launch and no copy more."""
        from ..utils.confidence import beam_score
        info = info or self.info
        if info is None:
            raise ValueError("dpmn_amd NativeASTER.read_conf: pass the AsterInfo of this vocabulary")
        self._check_eval()
        P = self._packs()
        rec, st = self.beam_search(self.encode(self.rectify(*self.prep(images), P)[1], P), return_stored=True, P=P)
        _, score, terms = beam_score(st["symbols"], st["predecessors"], st["scores"], rec.shape[0], BEAM, self.eos)
        return ids_to_strings(rec.numpy(), info), [float(v) for v in score], [int(v) for v in terms]

    @torch.no_grad()
    def read_lexicon(self, images, lex, info=None):
        """-> (greedy strings, the lexicon's strings, distances): `read`'s strings, then per string the lexicon word at the least
        edit distance (ops.edit_read: the strings packed and uploaded, dpmn_edit_lexicon_i32, one copy back).  An attention decoder
        has no frame posteriors, so lex.mode 'score' is refused."""
        if lex.mode == "score":
            raise ValueError("dpmn_amd NativeASTER.read_lexicon: the CTC score protocol needs a CTC recogniser (--rec crnn); use mode 'edit'")
        greedy = self.read(images, info)
        return (greedy,) + ops.edit_read(greedy, lex, images.device)
