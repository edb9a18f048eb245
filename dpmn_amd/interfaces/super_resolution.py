"""Mirror of ``interfaces/super_resolution.py::TextSR`` for the SR hot path.

``refine`` is the forward stack shared by eval()/test() in the reference (super_resolution.py:370-449 /
628-704): frozen PSN -> branch 1 (text-prior PGRMs) -> branch 2 (mask-prior PGRMs) -> CMM -> alpha
blend with the PSN image.  Every tensor op of the SR path runs in libdpmn_hip.so.  Text priors come from a callable
(``text_prior_fn(cascade_images, k) -> (B,2,H,W)`` uint8-valued floats, quirk Q6): by default the batched VisionLAN +
glyph-atlas pipeline of interfaces/text_prior.py (--rec_path), or seeded noise priors with
--synthetic_prior.  On real TextZoom data (dataset/textzoom.py) --arch tatt gets its label_vecs from the frozen CRNN mirror
(model/crnn.py, super_resolution.py:165-169).
"""
import contextlib
import csv
import os

import torch
from .. import _streams

from . import base
from .. import ops
from ..model.cmm import ComplementationModulationModule
from ..utils import synth


TRAIN_BRANCH_STREAMS = os.environ.get("DPMN_TRAIN_BRANCH_STREAMS", "1") != "0"
BRANCH_STREAMS = os.environ.get("DPMN_BRANCH_STREAMS", "1") != "0"      # 0: branch 1 and branch 2 of refine() on one stream
EVAL_PIPELINE = os.environ.get("DPMN_EVAL_PIPELINE", "1") != "0"        # 0: TextSR.eval / test run one batch at a time
GRAPH_MULTISTREAM = os.environ.get("DPMN_GRAPH_MULTISTREAM", "1") != "0"    # 0: graphed_train_step captures the step on ONE stream
DISTILL_ON_BRANCH = os.environ.get("DPMN_DISTILL_ON_BRANCH", "1") != "0"      # 0: the DistillModules run on the main stream before the CMM


_SIDE_STREAMS = {}


def side_streams(device):
    """The two branch streams that belong to the CURRENT stream of a device, shared by every TextSR object of the process (per-stream
    workspaces and allocator pools are then warmed once).  One pair per main stream: batches that run concurrently on different
    lanes (RefinePipeline) must not meet on a shared branch stream."""
    fixed = _streams.pool(device)          # (creates the training step's streams first: dpmn_amd/_streams.py)
    cur = torch.cuda.current_stream(device)
    if cur == torch.cuda.default_stream(device):
        return fixed["branch"]
    key = (device.type, device.index, cur.cuda_stream)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = (torch.cuda.Stream(device), torch.cuda.Stream(device))
    return _SIDE_STREAMS[key]


class RefinePipeline:
    """Throughput mode of `TextSR.refine` for a stream of INDEPENDENT batches (eval / test loops, serving): `depth` lanes, each a HIP
    stream with its own pair of branch streams; batch i runs on lane i % depth.  A batch has two single-stream phases -- the frozen
    PSN before the two branches fork and the CMM after they join -- whose launch-, ramp- and tail-bound kernels leave CUs idle; with
    two batches in flight those phases overlap the other batch's work (measured at B = 48: 8.31 -> 7.72 ms per batch).  Results are
    the same tensors `refine` returns (every module keeps one workspace per stream); a lane's work is ordered behind the caller's
    current stream at submit time, and `out.record_stream` / `wait(out)` order the caller behind the lane.
    Not for training: consecutive optimisation steps depend on each other."""

    def __init__(self, sr, model_list, model_psn, depth=2):
        assert depth >= 1
        self.sr, self.models, self.psn = sr, model_list, model_psn
        dev = next(model_list[-1].parameters()).device
        _streams.pool(dev)
        self.lanes = [torch.cuda.Stream(dev) for _ in range(depth)]
        self.events = [None] * depth
        self.i = 0

    def submit(self, images_lr, label_vecs=None, text_prior_fn=None, text_priors=None):
        """Enqueue one batch; returns its output tensor (complete when the lane reaches it: `wait(out)` or `synchronize()`)."""
        k = self.i % len(self.lanes)
        self.i += 1
        lane = self.lanes[k]
        lane.wait_stream(torch.cuda.current_stream(lane.device))      # the inputs were produced on the caller's stream
        with torch.cuda.stream(lane):
            out = self.sr.refine(self.models, self.psn, images_lr, label_vecs, text_prior_fn=text_prior_fn, text_priors=text_priors)
            ev = torch.cuda.Event()
            ev.record(lane)
        self.events[k] = ev
        out._dpmn_ready = ev
        return out

    @staticmethod
    def wait(out):
        """Order the caller's current stream behind the batch that produced `out`."""
        ev = getattr(out, "_dpmn_ready", None)
        if ev is not None:
            torch.cuda.current_stream(out.device).wait_event(ev)
            out.record_stream(torch.cuda.current_stream(out.device))
        return out

    def synchronize(self):
        for lane in self.lanes:
            lane.synchronize()


class _CombineLosses(torch.autograd.Function):
    """100 * sum(terms) / n over 0-d loss terms as ONE autograd node: cat + sum + mul + div forward, div + mul backward (every term gets
    the same gradient 100 g / n, computed once).  The reference's chain `loss += term.mean() * 100` ... `loss / n`
    (super_resolution.py:205-262) is three tiny launches per term forward and two to three backward: ~55 of the step's ~115 torch ops."""

    @staticmethod
    def forward(ctx, n, *terms):
        ctx.n, ctx.k = n, len(terms)
        return torch.cat([t.reshape(1) for t in terms]).sum() * 100 / n

    @staticmethod
    def backward(ctx, g):
        gt = (g / ctx.n) * 100
        return (None,) + (gt,) * ctx.k


class TextSR(base.TextBase):
    def build_models(self, testing=False):
        """Model list in the reference's order (super_resolution.py:38-76): b1 PGRMs (mode=False), b2 PGRMs
        (mode=True), CMM last; plus the frozen PSN."""
        b1, b2 = self.args.stu_iter_b1, self.args.stu_iter_b2
        share = self.args.sr_share
        models = [self.generator_init(0, mode=False, hidden_size=3, testing=testing)['model']]
        if not share:
            for i in range(b1 - 1):
                models.append(self.generator_init(i + 1, mode=False, hidden_size=3, testing=testing)['model'])
        models.append(self.generator_init(b1, mode=True, hidden_size=3, testing=testing)['model'])
        if not share:
            for i in range(b1, b1 + b2 - 1):
                models.append(self.generator_init(i + 1, mode=True, hidden_size=3, testing=testing)['model'])
        psn = self.generator_init(0, psn=True)['model']
        for p in psn.parameters():
            p.requires_grad = False
        psn.eval()
        cmm = ComplementationModulationModule().to(self.device)
        if testing:
            # super_resolution.py:570-582: test() evaluates the trained CMM, model_best_cmm.pth next to the PGRM files
            if not (self.resume and os.path.isdir(self.resume)):
                raise RuntimeError("dpmn_amd: test() needs --resume <dir> holding model_best_{k}.pth and model_best_cmm.pth")
            path = os.path.join(self.resume, "model_best_cmm.pth")
            if not os.path.isfile(path):
                raise FileNotFoundError("dpmn_amd: %s is missing -- refusing to evaluate a randomly initialised CMM" % path)
            print('loading pre-trained model from %s ' % path)
            sd = torch.load(path, map_location=self.device)['state_dict_G']
            cmm.load_state_dict({(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()})
        models.append(cmm)
        return models, psn

    def recogniser_text_prior(self, n=None, path=None, allow_random=False):
        """The reference's branch-1 prior source (super_resolution.py:100-111, 174-199): one VisionLAN per stage, driving the
        batched GPU pipeline of interfaces/text_prior.py.  path: the reference's --rec_path directory (recognizer_best_{i}.pth
        per stage) or one visionlan.pth-style file; without one this raises unless allow_random (tests / synthetic benches)."""
        from .text_prior import VisionLANTextPrior, build_recognizers
        n = self.args.stu_iter_b1 if n is None else n
        recs = build_recognizers(n, self.device, path if path is not None else self.rec_path, allow_random=allow_random)
        return VisionLANTextPrior(recs, self.device, font_path=getattr(self.args, "font_path", None))

    def default_text_prior(self):
        """--synthetic_prior (ours): seeded uint8-valued noise priors; otherwise the recogniser-driven prior (--tpg visionlan)."""
        if getattr(self.args, "synthetic_prior", True) or getattr(self.args, "tpg", "visionlan") != "visionlan":
            return self.synthetic_text_prior()
        return self.recogniser_text_prior()

    @staticmethod
    def synthetic_text_prior(seed=2):
        def fn(cascade, k):
            B, _, H, W = cascade.shape
            return torch.floor(synth.uniform("text_prior_%d" % k, (B, 2, H, W), 0.0, 256.0, seed)).to(cascade.device)
        return fn

    @torch.no_grad()
    def refine(self, model_list, model_psn, images_lr, label_vecs=None, text_prior_fn=None, text_priors=None,
               return_all=False):
        """super_resolution.py:370-449.  text_priors: optional precomputed list of b1 tensors (B,2,H,W)."""
        b1, b2 = self.args.stu_iter_b1, self.args.stu_iter_b2
        share = self.args.sr_share
        if self.args.arch in ('tsrn', 'tbsrn', 'tg'):
            images_lr_psn = model_psn(images_lr)
        elif self.args.arch == 'tatt':
            images_lr_psn, _ = model_psn(images_lr, label_vecs)
        elif self.args.arch == 'tpgsr':      # super_resolution.py:372-377: the PSN takes the recogniser's probabilities, returns the image
            images_lr_psn = model_psn(images_lr, label_vecs)
        else:
            raise NotImplementedError(self.args.arch)
        branch1, branch2 = [], []

        def run_branch1():
            cascade = images_lr_psn
            for k in range(b1):
                x_q = text_priors[k] if text_priors is not None else text_prior_fn(cascade, k)
                x_kv = cascade[:, :3]
                sr = model_list[0 if share else k](x_q, x_kv, branch1[:k])
                branch1.append(sr)
                cascade = sr

        def run_branch2():
            cascade = images_lr_psn
            for k in range(b1, b1 + b2):
                x_q = ops.to_mask(cascade)                      # batched toMask (util.py:27-35) on the GPU
                x_kv = cascade[:, :3]
                sr = model_list[0 if share else k](x_q, x_kv, branch2[:(k - b2)])   # slice quirk Q11
                branch2.append(sr)
                cascade = sr

        # The two branches only meet in the CMM: they run on two HIP streams, so that one branch's launch-, ramp- and tail-bound
        # kernels (the K = 96 GEMMs, gate, patch embedding: a third of a PGRM's launches) overlap the other branch's work.  Shared
        # modules (--sr_share) own ONE workspace and stay on one stream.
        if BRANCH_STREAMS and not share and images_lr.is_cuda:
            cur = torch.cuda.current_stream()
            s1, s2 = self._side_streams = side_streams(images_lr.device)
            s1.wait_stream(cur)
            s2.wait_stream(cur)
            with torch.cuda.stream(s1):
                run_branch1()
            with torch.cuda.stream(s2):
                run_branch2()
            cur.wait_stream(s1)
            cur.wait_stream(s2)
            for t_ in branch1 + branch2:
                t_.record_stream(cur)
        else:
            run_branch1()
            run_branch2()
        fused = model_list[-1](branch1[-1], branch2[-1])
        out = ops.blend(fused, images_lr_psn, self.args.alpha)
        if return_all:
            return out, dict(psn=images_lr_psn, branch1=branch1, branch2=branch2, cmm=fused)
        return out

    @torch.no_grad()
    def eval(self, model_list, val_loader, index=0, rec=None, aster_info=None, rec_list=None, model_psn=None, crnn_psn=None,
             text_prior_fn=None, display=False, display_failures=False, lexicon=None, beam=None):
        """super_resolution.py:340-513.  PSNR/SSIM always; recognition accuracy (lines 453-493) only when `rec` reads the SR images
        and the loader yields label strings as a 4th item: `rec` is the native CRNN (TextBase.CRNN_init, --rec crnn: its `read`), the
        native ASTER (TextBase.Aster_init, --rec aster: its `read`), the native MORAN (TextBase.MORAN_init, --rec moran: its `read`, the
        L2R decoder's strings cut at '$') or any callable images (B,3,H,W) -> list[str].  Without a recogniser 'accuracy' is None
        ("not computed"), never a fake 0.0.
        display=True (opt-in here; always on in the reference, line 505): after the loop the LAST batch's LR / SR / HR images are
        written by tripple_display under <vis_dir>/<index>/, named by the recogniser's strings of the LR and SR batch and the label
        (one extra recogniser call, on that batch's LR images; empty strings without a recogniser or labels).  display_failures=True
        (test(display=True); the call the reference has commented out at line 762): test_display on EVERY batch -- one more
        recogniser call per batch for the LR strings -- and their total under the key 'visualized'.  With both off nothing is
        written, no extra recogniser call is made and the returned dict has the keys it always had.
        lexicon (ours; an ops.Lexicon, main.py --rec_lexicon): the SR images are also read under the lexicon -- a native recogniser's
        read_lexicon (the CRNN: the word of the highest CTC likelihood, in the same forward pass; ASTER / MORAN: the word nearest to
        the greedy string), a plain callable's strings through ops.edit_read -- and the dict gains 'accuracy_lexicon', counted like
        'accuracy' (None when nothing was labelled or there is no recogniser).  'accuracy' and everything else are what they are
        without it.
        beam (ours; main.py --rec_beam / --rec_lm; utils/beam.py): a dict or an object with lm (an ops.CharLM or None), width, alpha,
        beta.  The SR images are also read by the CTC prefix beam search (rec.read_beam: the native CRNN, in the same forward pass as
        the greedy read; with a lexicon too, one pass more) and the dict gains 'accuracy_lm', counted exactly as 'accuracy_lexicon'."""
        from ..utils.util import str_filt
        from ..model.native import PackedEval
        reader = rec.read if isinstance(rec, PackedEval) and hasattr(rec, "read") else (rec if callable(rec) else None)
        lex_reader = self._lexicon_reader(rec, reader, lexicon)
        beam_reader = self._beam_reader(rec, reader, beam)
        for m in model_list:
            m.eval()
        fn = text_prior_fn or self.default_text_prior()
        psnr, ssim, n = [], [], 0
        n_correct, n_labelled, n_correct_lex, n_correct_lm = 0, 0, 0, 0
        last, visualized = None, 0      # display: (images_lr, sr, images_hr, LR strings | None, SR strings | None, labels | None) of the last batch
        # the batches of an evaluation pass are independent: two of them in flight (RefinePipeline).  The loop is software-pipelined:
        # batch i + 1 is prepared and SUBMITTED before this stream waits for batch i and queues its metrics -- a lane is ordered
        # behind this stream at submit time, so metrics queued before the submit would chain the lanes one after the other
        # (not with the recogniser-driven prior: the VisionLAN mirrors keep one set of activations per module, not per stream)
        pipe = None
        if EVAL_PIPELINE and self.device.type == "cuda" and not self.args.sr_share and not hasattr(fn, "recognizers"):
            key = (tuple(id(m) for m in model_list), id(model_psn))
            cached = getattr(self, "_eval_pipe", None)
            if cached is None or cached[0] != key:      # one pipeline (lane + branch streams, hence one workspace set) per model list
                cached = self._eval_pipe = (key, RefinePipeline(self, model_list, model_psn, 2))
            pipe = cached[1]

        def finish(sr, images_hr, labels, images_lr):
            nonlocal n, n_correct, n_labelled, n_correct_lex, n_correct_lm, last, visualized
            if pipe is not None:
                RefinePipeline.wait(sr)      # (the display kernels below read sr on this stream: behind the batch's lane)
            p, s = ops.psnr_ssim(sr, images_hr)
            psnr.append(p)
            ssim.append(s)
            n += sr.shape[0]
            preds_sr = preds_lr = None
            if reader is not None and labels is not None:      # (the host sync of the read: batch i + 1 is already submitted)
                if lex_reader is not None:
                    preds_sr, preds_lex, _ = lex_reader(sr[:, :3])
                    for pred, target in zip(preds_lex, labels):
                        n_correct_lex += int(pred == str_filt(target, 'lower'))
                elif beam_reader is None:
                    preds_sr = reader(sr[:, :3])
                if beam_reader is not None:      # (without a lexicon the greedy strings come from the same pass)
                    greedy, preds_lm, _ = beam_reader(sr[:, :3])
                    preds_sr = greedy if preds_sr is None else preds_sr
                    for pred, target in zip(preds_lm, labels):
                        n_correct_lm += int(pred == str_filt(target, 'lower'))
                for pred, target in zip(preds_sr, labels):
                    n_correct += int(pred == str_filt(target, 'lower'))
                n_labelled += len(labels)
                if display_failures:
                    preds_lr = reader(images_lr[:, :3])
                    visualized += self.test_display(images_lr, sr, images_hr, preds_lr, preds_sr, labels, str_filt)
            if display:
                last = (images_lr, sr, images_hr, preds_lr, preds_sr, labels)

        pending = None
        for data in val_loader:
            images_hr, images_lr = data[0].to(self.device), data[1].to(self.device)
            label_vecs = data[2].to(self.device) if len(data) > 2 and data[2] is not None else None
            if label_vecs is None and self.args.arch in ('tatt', 'tpgsr'):      # real data: TATT's label_vecs come from the frozen CRNN (lines 165-169)
                label_vecs = self.label_vecs_from_crnn(images_lr)
            if getattr(self.args, "rotate_test", 0):      # super_resolution.py:358-365 (angle range from rotate_train, as there)
                images_lr, images_hr = self.rotate_pair(images_lr, images_hr, self.args.rotate_train)
            labels = data[3] if len(data) > 3 else None
            if pipe is not None:
                sr = pipe.submit(images_lr, label_vecs, text_prior_fn=fn)
                if pending is not None:
                    finish(*pending)
                pending = (sr, images_hr, labels, images_lr)
            else:
                finish(self.refine(model_list, model_psn, images_lr, label_vecs, fn), images_hr, labels, images_lr)
        if pending is not None:
            finish(*pending)
        if display and last is not None:      # super_resolution.py:505, once per pass, on the last batch
            images_lr, sr, images_hr, preds_lr, preds_sr, labels = last
            blank = [''] * images_lr.shape[0]
            if preds_lr is None and preds_sr is not None:
                preds_lr = reader(images_lr[:, :3])      # super_resolution.py:461-489: the same recogniser on the LR batch
            self.tripple_display(images_lr, sr, images_hr, preds_lr or blank, preds_sr or blank, labels if labels is not None else blank, index)
        psnr_avg = float(torch.stack(psnr).mean().item())
        ssim_avg = float(torch.stack(ssim).mean().item())
        accuracy = round(n_correct / n_labelled, 4) if n_labelled else None
        res = {'psnr': psnr, 'ssim': ssim, 'accuracy': accuracy, 'psnr_avg': round(psnr_avg, 6), 'ssim_avg': round(ssim_avg, 6)}
        if display_failures:
            res['visualized'] = visualized
        if lexicon is not None:
            res['accuracy_lexicon'] = round(n_correct_lex / n_labelled, 4) if n_labelled and lex_reader is not None else None
        if beam is not None:
            res['accuracy_lm'] = round(n_correct_lm / n_labelled, 4) if n_labelled and beam_reader is not None else None
        return res

    @staticmethod
    def _beam_settings(beam):
        """eval / demo's `beam` (a dict or an object with lm, width, alpha, beta; missing ones take read_beam's defaults) -> the
        keywords of read_beam."""
        get = beam.get if isinstance(beam, dict) else (lambda k, d=None: getattr(beam, k, d))
        return {"lm": get("lm"), "width": int(get("width", 16)), "alpha": float(get("alpha", 0.5)), "beta": float(get("beta", 0.0))}

    @classmethod
    def _beam_reader(cls, rec, reader, beam):
        """eval / demo: images -> (greedy strings, the beam search's strings, scores), or None without `beam` or a recogniser.  The
        search needs frame posteriors: a recogniser without read_beam (ASTER, MORAN, a plain callable) is a ValueError."""
        if beam is None or reader is None:
            return None
        if not callable(getattr(rec, "read_beam", None)):
            raise ValueError("the CTC beam search needs a CTC recogniser with read_beam (NativeCRNN, --rec crnn); ASTER and MORAN have their "
                             "own decoders")
        kw = cls._beam_settings(beam)
        return lambda images: rec.read_beam(images, **kw)

    @staticmethod
    def _with_beam(lex_reader, beam_reader):
        """demo: one reader for the lexicon's and the beam search's columns: images -> (greedy strings, [the lexicon's strings, their
        scores,] the beam search's strings, their scores).  Without a lexicon it is read_beam's one pass."""
        if lex_reader is None:
            return beam_reader

        def read(images):
            return tuple(lex_reader(images)) + tuple(beam_reader(images)[1:])
        return read

    @staticmethod
    def _lexicon_reader(rec, reader, lexicon):
        """eval / demo: images -> (greedy strings, the lexicon's strings, scores) for a recogniser resolved to `reader`, or None
        without a lexicon or a recogniser.  A native recogniser brings its own read_lexicon; any other callable's strings take the
        edit protocol (ops.edit_read)."""
        if lexicon is None or reader is None:
            return None
        if hasattr(rec, "read_lexicon"):
            return lambda images: rec.read_lexicon(images, lexicon)
        if lexicon.mode == "score":
            raise ValueError("the CTC score protocol of a lexicon needs a CTC recogniser (NativeCRNN); a callable recogniser takes mode 'edit'")

        def read(images):
            strings = list(reader(images))
            return (strings,) + ops.edit_read(strings, lexicon, images.device)
        return read

    @torch.no_grad()
    def demo(self, model_list, model_psn, batches, out_dir, rec=None, text_prior_fn=None, tile=False, chunk=None, boxes=False, paste=False,
             feather=1.0, paste_polygons=False, lexicon=None, confidence=False, upright=False, min_conf=None, line_read=False, line_space=0,
             lexicon_penalty=0.0, beam=None):
        """Super-resolve someone's own images (ours; main.py --demo_dir): batches yields (names, images_lr) as
        dataset.folder.folder_batches does.  Per batch `refine` (label_vecs from the frozen CRNN for tatt / tpgsr, as in eval), then
        save_image's quantisation on the GPU (ops.quantize_sr_u8), ONE device-to-host copy and one <stem>_sr.png per input under
        out_dir.  With a recogniser (resolved as in eval) the strings it reads from the LR input and from the SR image go into
        out_dir/demo_result.csv: a header and one row file, lr_string, sr_string per image (empty strings without one).  A name whose
        stem is taken (a.png after a.jpg) keeps its extension: a.png_sr.png.  Returns the rows.
        A batch of ONE image changes SKConv's squeeze() semantics (quirk Q3; base.py _loader guards the loaders against it): it runs
        with the image repeated and the duplicate's output dropped.
        tile=True (main.py --demo_tile): batches yields (names, plan, images_lr) as dataset.folder.folder_window_batches does -- every
        image as overlapping LR windows of its line.  The windows of a batch go through `refine` in chunks of at most `chunk` windows
        (default: the batch size; a chunk of one window is repeated as above, label_vecs per window), ops.stitch_windows_u8 blends the
        SR windows of an image on the GPU, and <stem>_sr.png is scale * lr_h high and scale * w_line wide.  lr_string / sr_string are
        then the reads of the image's WINDOWS joined with '|': a recogniser sees lr_w columns at a time and neighbouring windows
        overlap, so this is not a transcription of the line.  An image of one window is written as without tile.
        boxes=True (main.py --demo_boxes): the inputs are the text regions of whole photos; batches yields (names, labels, images_lr)
        as dataset.folder.box_region_batches does -- with tile=True (names, labels, plan, images_lr) as box_window_batches does --
        names being the region names <stem>_<k>.  A photo is never split, so a batch may hold more regions than the batch size: they
        go through `refine` in chunks of at most `chunk` (default: the batch size; a chunk of one is repeated as above).  One
        <stem>_<k>_sr.png per region; demo_result.csv then has the header file, box, label, lr_string, sr_string: the photo's stem,
        the region's number k, its transcription from the box file.  Without boxes nothing changes.
        paste=True (main.py --demo_paste; needs boxes=True): the batches come from the same generators with photos=True, so every tuple
        ends with the batch's uploaded photos and quadrilaterals.  Once a batch's regions are super-resolved, each of its photos is
        enlarged by the scale factor on the GPU (ops.resize_ragged_u8 at the photo's own target size: PIL's bytes), its SR regions --
        the very bytes of the <stem>_<k>_sr.png files, still on the device -- are pasted into their quadrilaterals in box-file order
        (ops.paste_mixed_u8, utils/paste.py; feather: the width of the blended edge in SR pixels, 0 for a hard edge), and the photo
        is copied to the host once and written as <stem>_photo_sr.png.  A photo whose enlarged side would exceed
        utils.resize.MAX_SIDE gets one printed line and no photo output; its regions are written.  The rows and demo_result.csv do
        not change.
        Batches made with polygons=True (main.py --demo_polygons) need nothing here: a rectified polygon (utils/poly.py) is a region
        like any other, with or without tile.  With paste=True the polygons' SR regions are written as files but not pasted, unless
        paste_polygons=True (main.py --demo_paste_polygons; needs paste=True): every strip of a polygon's SR region then goes back into
        its piece of the enlarged photo by the inverse of the strip's bilinear map (utils/paste_poly.py), and quadrilaterals and
        polygons are pasted from one list in box-file order (ops.paste_mixed_u8).  The region files and demo_result.csv do not change.
        lexicon (an ops.Lexicon, main.py --rec_lexicon; needs a recogniser, not with tile: a window is not a word): the SR image is
        also read under the lexicon (as in eval) and every row and demo_result.csv gain the columns sr_lexicon, sr_lexicon_score after
        sr_string: the lexicon's word and its CTC log-likelihood (the CRNN's score protocol) or its edit distance to sr_string.
        confidence / upright / min_conf (ours; main.py --demo_conf, --demo_upright, --demo_min_conf; utils/confidence.py; not with
        tile): rec must be an object with read_conf(images) -> (strings, scores, terms) -- the native recognisers, or a stub; a plain
        callable returns no score and is refused.  Every read then comes from read_conf, and with any of the three the rows gain
        lr_conf after lr_string and sr_conf after sr_string (exp(score / terms), written with %.4f).
        upright: every LR batch is read twice on the device, as it is and through ops.turn180 (the mask channel turns along);
        utils.confidence.choose_direction picks per image, and the chosen tensor is what `refine`, the region file and sr_string see
        (one more recogniser pass per LR batch, no SR pass more).  lr_string / lr_conf are the chosen direction's, and a column turned
        (0 / 1) follows sr_conf.  With paste a turned region goes into its quadrilateral with the corner list rotated by two (a
        polygon of 2k points: by k), so the pixels land where they were cut.
        min_conf C (0 < C < 1; needs boxes): a region whose sr_string is empty or whose sr_conf < C is dropped -- no region file, not
        pasted -- and its row stays, with a last column kept = 0 (1 otherwise); one printed line per photo gives the dropped count.
        With boxes, upright or min_conf write out_dir/boxes_read/<stem>.txt: the kept regions in box-file order, the corners in the
        chosen reading order, sr_string as the transcription -- a box file for a second run.  The corner lists come with the batches:
        they must then be made with photos=True, whether paste is set or not.
        The columns, in order: file, [box, label,] lr_string, lr_conf, sr_string, sr_conf, [turned,] [sr_lexicon, sr_lexicon_score,]
        [kept]; the lexicon's read of the SR image stays a second call through read_lexicon.  Without the three nothing changes.
        beam (ours; main.py --rec_beam / --rec_lm; utils/beam.py; eval's setting: lm, width, alpha, beta; needs a recogniser with
        read_beam -- NativeCRNN; not with tile: a line has word boundaries that the CRNN has no class for): the SR image is also read by
        the CTC prefix beam search with the character model and the rows gain sr_lm, sr_lm_score (the string and its float64 score,
        %.6g).  With every option the columns are, in order: file, [box, label,] lr_string, [lr_conf,] sr_string, [sr_conf,] then
        EITHER (with a lexicon) [turned,] sr_lexicon, sr_lexicon_score, sr_lm, sr_lm_score OR (without one) sr_lm, sr_lm_score,
        [turned,] and last [kept]: sr_lm follows the lexicon's columns where they are, else sr_string or sr_conf.  Without a lexicon
        the greedy strings come from read_beam's own pass; with one, read_beam is one call more.
        line_read (ours; main.py --demo_line_read; utils/line_read.py; needs tile=True and a CTC recogniser with window_rows and
        read_lines -- NativeCRNN; ASTER and MORAN have no frame posteriors): lr_string / sr_string are ONE read of the whole line per
        side, with no '|': the frame posteriors of the line's windows are kept on the device chunk by chunk, blended along the line
        with the pixel stitch's ramp in the log domain, decoded once and scored once (three launches and one device-to-host copy
        per side and batch; the recogniser runs as often as without the flag).  An image of one window gets `read`'s string.  The
        blend cannot repair a glyph that both windows see cut, and the string is over the CRNN's 36 symbols.  line_space N (0 ..
        64): a space goes where at least N line frames lie between two symbols' arg-max runs -- a heuristic on the blank runs, the
        CRNN has no space class; 0 inserts none.  With line_read, confidence=True combines with tile: lr_conf / sr_conf are
        exp(score / terms) of the line's CTC likelihood; upright and min_conf stay refused with tile.  The <stem>_sr.png files do
        not change.
        lexicon with tile=True and line_read=True (ours; main.py --rec_lexicon with --demo_tile --demo_line_read;
        utils/line_words.py; the lexicon's mode None or 'score', rec with read_lines): the SR line's stitched posteriors are also
        decoded as a sequence of the lexicon's words -- the one-pass Viterbi over "blank gap, word, blank gap, ...", in the same
        read_lines call and the same host copy -- and sr_lexicon / sr_lexicon_score are the words joined by single spaces and the
        line's Viterbi score.  lexicon_penalty (finite, default 0.0, untuned): added once per word; negative means fewer, longer
        words.  Every frame must be explained by a lexicon word or a gap, so a word outside the list comes back as its
        nearest-scoring neighbours (sr_string beside it stays the open-vocabulary read), and two words need a blank frame between
        them.  Without line_read a lexicon stays refused with tile."""
        from ..model.native import PackedEval
        reader = rec.read if isinstance(rec, PackedEval) and hasattr(rec, "read") else (rec if callable(rec) else None)
        if lexicon is not None and tile and not line_read:
            raise ValueError("demo: a lexicon does not combine with tile=True (a window of a line is not a word)")
        if lexicon is not None and reader is None:
            raise ValueError("demo: a lexicon needs a recogniser")
        line_kw = self._line_reader(rec, tile, line_read, line_space)
        if lexicon is not None and line_kw:
            # (a tiled line under a lexicon: the SR line's stitched posteriors are decoded as a sequence of its words)
            import math
            if lexicon.mode == "edit":
                raise ValueError("demo: a lexicon in mode 'edit' does not combine with tile=True and line_read=True (the line's words "
                                 "come from its frame posteriors)")
            if not math.isfinite(float(lexicon_penalty)):
                raise ValueError("demo: lexicon_penalty must be finite, got %r" % (lexicon_penalty,))
            line_kw = dict(line_kw, lexicon=lexicon, penalty=float(lexicon_penalty))
        elif lexicon_penalty:
            raise ValueError("demo: lexicon_penalty needs a lexicon and line_read=True (it is the per-word score of a line's lexicon read)")
        lex_reader = self._lexicon_reader(rec, reader, lexicon) if not line_kw else None
        if beam is not None and tile:
            raise ValueError("demo: the CTC beam search does not combine with tile=True (a line has word boundaries that the CRNN has no "
                             "class for, and a window of a line is not a word)")
        if beam is not None and reader is None:
            raise ValueError("demo: the CTC beam search needs a recogniser")
        beam_reader = self._beam_reader(rec, reader, beam)
        lm_kw = {}
        if beam_reader is not None:
            # (from here the lexicon's item holds the beam search's two lists behind the lexicon's two, or alone)
            lex_reader, lm_kw = self._with_beam(lex_reader, beam_reader), {"lm": True}
        # (with line_read the confidence columns are the lines' own: no read_conf, and nothing else of the three combines with tile)
        conf_reader = self._conf_reader(rec, tile, boxes, confidence and not line_kw, upright, min_conf)
        line_conf = bool(line_kw) and bool(confidence)
        for m in model_list:
            m.eval()
        fn = text_prior_fn or self.default_text_prior()
        os.makedirs(out_dir, exist_ok=True)
        rows, taken = [], set()
        if paste and not boxes:
            raise ValueError("demo: paste=True needs boxes=True (the quadrilaterals the SR regions are pasted into come from the box files)")
        if paste_polygons and not paste:
            raise ValueError("demo: paste_polygons=True needs paste=True (the polygons are pasted into the photo that paste=True writes)")
        if boxes:
            labels = []
            conf_kw = {} if conf_reader is None else dict(conf_reader=conf_reader, upright=bool(upright), min_conf=min_conf, out_dir=out_dir)
            for names, pixels, preds_lr, preds_sr, photos, *lex in self._demo_regions(model_list, model_psn, batches, fn, reader, chunk, tile, labels,
                                                                                       float(feather) if paste else None, bool(paste_polygons),
                                                                                       lex_reader, **conf_kw, **self._line_kw(line_kw, line_conf)):
                if conf_reader is not None:      # lex = [the lexicon's item or None, (lr_conf, sr_conf, turned or None), kept or None]
                    self._demo_write(out_dir, [n + ".png" for n in names], pixels, preds_lr, preds_sr, rows, taken, lex[0], conf=lex[1], kept=lex[2],
                                     **lm_kw)
                else:
                    self._demo_write(out_dir, [n + ".png" for n in names], pixels, preds_lr, preds_sr, rows, taken, *lex, **lm_kw)
                self._demo_write(out_dir, [stem + "_photo.png" for stem, _ in photos], [a for _, a in photos], [''] * len(photos),
                                 [''] * len(photos), [], taken)
            # <stem>_<k>.png, lr, sr -> stem, k, label, lr, sr
            rows = [r[0][:-4].rsplit("_", 1) + [label] + r[1:] for r, label in zip(rows, labels)]      # (+ the lexicon's two columns)
            batches = ()
        elif tile:
            for names, pixels, preds_lr, preds_sr, _, conf, lex in self._demo_windows(model_list, model_psn, batches, fn, reader, chunk, line_kw):
                self._demo_write(out_dir, names, pixels, preds_lr, preds_sr, rows, taken, lex, conf=conf + (None,) if line_conf else None)
            batches = ()
        for names, images_lr in batches:
            n = len(names)
            images_lr = images_lr.to(self.device)
            if conf_reader is not None:
                images_lr, preds_lr, conf_lr, turned = self._demo_upright(conf_reader, images_lr, upright)
            if n == 1:
                images_lr = torch.cat([images_lr, images_lr], 0)
            label_vecs = self.label_vecs_from_crnn(images_lr) if self.args.arch in ('tatt', 'tpgsr') else None
            sr = self.refine(model_list, model_psn, images_lr, label_vecs, fn)[:n]
            pixels = ops.quantize_sr_u8(sr).cpu().numpy()
            if conf_reader is not None:
                preds_sr, conf_sr = conf_reader(sr[:, :3])
                self._demo_write(out_dir, names, pixels, preds_lr, preds_sr, rows, taken, lex_reader(sr[:, :3])[1:] if lex_reader is not None else None,
                                 conf=(conf_lr, conf_sr, turned if upright else None), **lm_kw)
                continue
            blank = [''] * n
            preds_lr = reader(images_lr[:n, :3]) if reader is not None else blank
            if lex_reader is not None:
                preds_sr, *lex = lex_reader(sr[:, :3])
                self._demo_write(out_dir, names, pixels, preds_lr, preds_sr, rows, taken, lex, **lm_kw)
                continue
            preds_sr = reader(sr[:, :3]) if reader is not None else blank
            self._demo_write(out_dir, names, pixels, preds_lr, preds_sr, rows, taken)
        with open(os.path.join(out_dir, "demo_result.csv"), "w", newline="") as out:
            w = csv.writer(out)
            head = ["file", "box", "label"] if boxes else ["file"]
            lm_head = ["sr_lm", "sr_lm_score"] if beam_reader is not None else []
            if conf_reader is None and not line_conf:
                head += ["lr_string", "sr_string"]
            else:      # (without a lexicon sr_lm follows sr_conf, before turned)
                head += ["lr_string", "lr_conf", "sr_string", "sr_conf"] + (lm_head if lexicon is None else []) + (["turned"] if upright else [])
                lm_head = lm_head if lexicon is not None else []
            w.writerow(head + (["sr_lexicon", "sr_lexicon_score"] if lexicon is not None else []) + lm_head
                       + (["kept"] if min_conf is not None else []))
            w.writerows(rows)
        return rows

    @staticmethod
    def _line_reader(rec, tile, line_read, line_space):
        """demo: None without line_read, else _demo_windows' line_kw {rec, gap}.  ValueError of one line for line_read without tile or
        with a recogniser that has no frame posteriors, and for a line_space outside 0 .. 64 or without line_read."""
        gap = int(line_space or 0)
        if not line_read:
            if gap:
                raise ValueError("demo: line_space needs line_read=True (the spaces go into the one read of a tiled line)")
            return None
        if not tile:
            raise ValueError("demo: line_read needs tile=True (it reads a line that was super-resolved in overlapping windows as one string)")
        if not (callable(getattr(rec, "window_rows", None)) and callable(getattr(rec, "read_lines", None))):
            raise ValueError("demo: line_read needs a CTC recogniser with window_rows and read_lines (NativeCRNN, --rec crnn); ASTER and "
                             "MORAN have no frame posteriors to blend along a line")
        if not 0 <= gap <= 64:
            raise ValueError("demo: line_space must be 0 .. 64 line frames, got %r" % (line_space,))
        return {"rec": rec, "gap": gap}

    @staticmethod
    def _line_kw(line_kw, line_conf):
        """demo(boxes=True): _demo_regions' keywords for a line read; none without one."""
        return {"line_kw": line_kw, "line_conf": line_conf} if line_kw else {}

    @staticmethod
    def _conf_reader(rec, tile, boxes, confidence, upright, min_conf):
        """demo: images -> (strings, conf values) through rec.read_conf, or None without confidence / upright / min_conf.  ValueError
        of one line for the flags with tile, a recogniser without read_conf, min_conf without boxes or outside (0, 1)."""
        if not (confidence or upright or min_conf is not None):
            return None
        from ..utils.confidence import confidence as conf_of
        if tile:
            raise ValueError("demo: confidence, upright and min_conf do not combine with tile=True (a window of a line is not a word)")
        if not callable(getattr(rec, "read_conf", None)):
            raise ValueError("demo: confidence, upright and min_conf need a recogniser object with read_conf(images) -> (strings, scores, "
                             "terms); a plain callable returns no score")
        if min_conf is not None and not boxes:
            raise ValueError("demo: min_conf needs boxes=True (it drops regions of a photo; an image of a folder is not a candidate region)")
        if min_conf is not None and not 0.0 < float(min_conf) < 1.0:
            raise ValueError("demo: min_conf must lie in (0, 1), got %r" % (min_conf,))

        def read(images):
            strings, scores, terms = rec.read_conf(images)
            return [str(s) for s in strings], conf_of(scores, terms)
        return read

    @staticmethod
    def _demo_upright(conf_reader, x, upright):
        """demo: the LR read of a batch x (n, C, h, w) -> (the batch, its strings, its conf values, turned flags).  upright: the batch
        is also read through ops.turn180 and every image is taken in the direction utils.confidence.choose_direction picks."""
        from ..utils.confidence import choose_direction
        s_up, c_up = conf_reader(x[:, :3])
        if not upright:
            return x, s_up, c_up, [0] * len(s_up)
        xt = ops.turn180(x)
        s_t, c_t = conf_reader(xt[:, :3])
        turned = [choose_direction(cu, su, ct, st) for cu, su, ct, st in zip(c_up, s_up, c_t, s_t)]
        if any(turned):
            x = torch.where(torch.tensor(turned, device=x.device).view(-1, 1, 1, 1), xt, x)
        return (x, [st if t else su for t, su, st in zip(turned, s_up, s_t)], [ct if t else cu for t, cu, ct in zip(turned, c_up, c_t)],
                [int(t) for t in turned])

    @staticmethod
    def _demo_write(out_dir, names, pixels, preds_lr, preds_sr, rows, taken, lex=None, conf=None, kept=None, lm=False):
        """demo: one <stem>_sr.png per image of a batch and its row; lex: None, or (the lexicon's strings, their scores), two more
        columns.  conf: None, or (lr conf values, sr conf values, turned flags or None): the row's confidence columns.  kept: None,
        or one flag per image: an image that is not kept gets no file, and the row ends with the flag.  lm: the LAST two lists of lex
        are the beam search's (strings, scores) -- alone, or behind the lexicon's two; alone they stand before the turned flag."""
        from PIL import Image
        more = [[cell for k in range(0, len(t), 2) for cell in (str(t[k]), "%.6g" % t[k + 1])] for t in zip(*lex)] if lex is not None else [[]] * len(names)
        lm_first = bool(lm) and lex is not None and len(lex) == 2      # (no lexicon's columns to follow)
        for i, (name, a, s_lr, s_sr, extra) in enumerate(zip(names, pixels, preds_lr, preds_sr, more)):
            if kept is None or kept[i]:
                out_name = os.path.splitext(name)[0] + "_sr.png"
                if out_name in taken:
                    out_name = name + "_sr.png"
                while out_name in taken:
                    out_name = "_" + out_name
                taken.add(out_name)
                Image.fromarray(a).save(os.path.join(out_dir, out_name))
            if conf is None:
                rows.append([name, str(s_lr), str(s_sr)] + extra)
                continue
            turned = [str(int(conf[2][i]))] if conf[2] is not None else []
            rows.append([name, str(s_lr), "%.4f" % conf[0][i], str(s_sr), "%.4f" % conf[1][i]] + (extra + turned if lm_first else turned + extra)
                        + ([str(int(bool(kept[i])))] if kept is not None else []))

    def _demo_regions(self, model_list, model_psn, batches, fn, reader, chunk, tile, labels_out, feather=None, paste_polygons=False,
                      lex_reader=None, conf_reader=None, upright=False, min_conf=None, out_dir=None, line_kw=None, line_conf=False):
        """demo(boxes=True): per batch of regions -> (names, one (H, W_r, 3) uint8 array per region, the LR reads, the SR reads, the
        pasted photos); the regions' labels are appended to labels_out.  tile: the batches carry a plan and go through _demo_windows.
        feather: None, or demo(paste=True)'s -- the batches then end with the photos item and the pasted photos are _demo_paste's list
        (empty otherwise); paste_polygons: demo's.  lex_reader (demo's lexicon; not with tile): the SR regions are read through it
        and the tuple gets a sixth item, (the lexicon's strings, their scores).
        conf_reader (demo's confidence / upright / min_conf; not with tile): every read comes from it, the LR read through
        _demo_upright, and the tuple ends with three items: the lexicon's item or None, (lr conf values, sr conf values, turned flags
        or None), kept flags or None.  A turned region is pasted with its corner list rotated, a dropped one not at all; with upright or
        min_conf the batches carry the photos item and out_dir/boxes_read/<stem>.txt is written per photo."""
        from ..utils.confidence import box_line, rotate_corners
        paste = feather is not None
        if tile:
            held = []

            def windows():
                for names, labels, plan, images_lr, *photos in batches:
                    labels_out.extend(labels)
                    held[:] = photos
                    yield names, plan, images_lr
            for names, pixels, preds_lr, preds_sr, device, conf, lex in self._demo_windows(model_list, model_psn, windows(), fn, reader, chunk, line_kw):
                pasted = self._demo_paste(names, held[0], device[0], device[1], feather, paste_polygons) if paste else []
                if line_conf:      # (demo(line_read=True, confidence=True): the lexicon's item or None, the lines' conf values, nothing turned)
                    yield names, pixels, preds_lr, preds_sr, pasted, lex, conf + (None,)
                elif lex is not None:
                    yield names, pixels, preds_lr, preds_sr, pasted, lex
                else:
                    yield names, pixels, preds_lr, preds_sr, pasted
            return
        chunk = max(int(chunk if chunk is not None else self.batch_size), 1)
        for names, labels, images_lr, *photos in batches:
            labels_out.extend(labels)
            images_lr = images_lr.to(self.device)
            pixels, preds_lr, preds_sr, on_device = [], [], [], []
            lex = ([], [])
            conf_lr, conf_sr, turned = [], [], []
            for lo in range(0, images_lr.shape[0], chunk):
                x = images_lr[lo:lo + chunk]
                n = x.shape[0]
                if conf_reader is not None:
                    x, s_lr, c_lr, t = self._demo_upright(conf_reader, x, upright)
                    preds_lr += s_lr
                    conf_lr += c_lr
                    turned += t
                if n == 1:
                    x = torch.cat([x, x], 0)
                label_vecs = self.label_vecs_from_crnn(x) if self.args.arch in ('tatt', 'tpgsr') else None
                sr = self.refine(model_list, model_psn, x, label_vecs, fn)[:n]
                q = ops.quantize_sr_u8(sr)
                pixels.append(q.cpu().numpy())
                if paste:
                    on_device.append(q)
                if conf_reader is not None:
                    s_sr, c_sr = conf_reader(sr[:, :3])
                    preds_sr += s_sr
                    conf_sr += c_sr
                    if lex_reader is not None:
                        got = lex_reader(sr[:, :3])
                        lex = lex if len(lex) == len(got) - 1 else tuple([] for _ in got[1:])      # (two more lists with the beam search)
                        for held, new in zip(lex, got[1:]):
                            held.extend(new)
                    continue
                preds_lr += list(reader(x[:n, :3])) if reader is not None else [''] * n
                if lex_reader is not None:
                    got = lex_reader(sr[:, :3])
                    preds_sr += list(got[0])
                    lex = lex if len(lex) == len(got) - 1 else tuple([] for _ in got[1:])
                    for held, new in zip(lex, got[1:]):
                        held.extend(new)
                else:
                    preds_sr += list(reader(sr[:, :3])) if reader is not None else [''] * n
            pasted = []
            kept, skip = None, ()
            if conf_reader is not None and (upright or min_conf is not None):
                if not photos:
                    raise ValueError("demo: upright and min_conf with boxes=True need batches made with photos=True (they carry the corner "
                                     "lists that boxes_read is written from)")
                if min_conf is not None:
                    kept = [bool(s) and c >= float(min_conf) for s, c in zip(preds_sr, conf_sr)]
                    skip = {r for r, k in enumerate(kept) if not k}
                # (a turned region is read, and pasted, from its opposite corner)
                photos = [photos[0][:3] + ([rotate_corners(q) if t else q for q, t in zip(photos[0][3], turned)],)]
                os.makedirs(os.path.join(out_dir, "boxes_read"), exist_ok=True)
                stems = [name.rsplit("_", 1)[0] for name in names]
                for stem in sorted(set(stems), key=stems.index):
                    mine = [r for r, s in enumerate(stems) if s == stem]
                    with open(os.path.join(out_dir, "boxes_read", stem + ".txt"), "w", encoding="utf-8") as fh:
                        fh.writelines(box_line(photos[0][3][r], preds_sr[r]) + "\n" for r in mine if r not in skip)
                    if min_conf is not None:
                        print("demo: %d of %d regions of %s dropped (empty read or confidence below %g)"
                              % (sum(r in skip for r in mine), len(mine), stem, float(min_conf)))
            if paste:
                # the quantised regions of the batch, all H x W x 3: flat, they are pack_ragged's layout
                q = on_device[0] if len(on_device) == 1 else torch.cat(on_device, 0)
                R, H, W = q.shape[:3]
                pasted = self._demo_paste(names, photos[0], q.reshape(-1), [(r * H * W * 3, H, W) for r in range(R)], feather,
                                          paste_polygons, *((skip,) if skip else ()))
            if conf_reader is not None:
                yield (names, [a for p in pixels for a in p], preds_lr, preds_sr, pasted, lex if lex_reader is not None else None,
                       (conf_lr, conf_sr, turned if upright else None), kept)
                continue
            if lex_reader is not None:
                yield names, [a for p in pixels for a in p], preds_lr, preds_sr, pasted, lex
                continue
            yield names, [a for p in pixels for a in p], preds_lr, preds_sr, pasted

    def _demo_paste(self, names, photos, sr_packed, sr_meta, feather, paste_polygons=False, skip=()):
        """demo(paste=True): the photos of one batch with their SR regions pasted back -> [(stem, (scale * H, scale * W, 3) uint8
        array)] in batch order.  photos = (packed, meta, owners, quads) as dataset.folder.box_region_batches(photos=True) yields it;
        sr_packed / sr_meta hold the batch's SR regions on the device, one per name, in pack_ragged's layout.  Per photo: the enlargement
        (ops.resize_ragged_u8 with a batch of one), ops.paste_mixed_u8 with the photo's regions in box-file order, one copy to the
        host.  A photo too large to enlarge, or a region utils.paste.paste_coeffs refuses, is passed over with one printed line.  The
        regions of polygons (more than 4 points: the batches were made with polygons=True) are not pasted -- one printed line per photo
        gives their count -- unless paste_polygons: a polygon then joins the photo's list with its strip table
        (utils.paste_poly.strip_table; one it refuses gets a refused quadrilateral's printed line).  skip: the regions (indices into
        names) that demo's min_conf dropped; they are not pasted, and a photo all of whose regions were dropped is not written."""
        import numpy as np
        from ..utils.paste import paste_coeffs
        from ..utils.paste_poly import strip_table
        from ..utils.resize import MAX_SIDE
        packed, meta, owners, quads = photos
        meta = np.asarray(meta.cpu() if torch.is_tensor(meta) else meta).astype(np.int64).reshape(-1, 3)
        sr_meta = np.asarray(sr_meta, np.int64).reshape(-1, 3)
        s = int(self.scale_factor)
        out = []
        for b, (_, H, W) in enumerate(meta.tolist()):
            mine = [r for r, o in enumerate(owners) if o == b]
            if not mine:
                continue
            stem = names[mine[0]].rsplit("_", 1)[0]
            if skip:
                mine = [r for r in mine if r not in skip]
                if not mine:
                    continue
            if s * H > MAX_SIDE or s * W > MAX_SIDE:
                print("demo: no pasted photo for %s (%d x %d times %d: a side above %d is not resized)" % (stem, H, W, s, MAX_SIDE))
                continue
            curved = [r for r in mine if len(quads[r]) > 4]
            if curved and not paste_polygons:
                print("demo: %d polygon region%s of %s not pasted (only quadrilaterals are warped back)"
                      % (len(curved), "" if len(curved) == 1 else "s", stem))
            regions = []
            for r in mine:
                if r in curved and not paste_polygons:
                    continue
                try:
                    shape = strip_table if r in curved else paste_coeffs
                    regions.append((r, shape(quads[r], s, int(sr_meta[r, 2]), int(sr_meta[r, 1])), feather))
                except ValueError as e:
                    print("demo: region %s is not pasted (%s)" % (names[r], e))
            photo2 = ops.resize_ragged_u8(packed, meta[b:b + 1], s * H, s * W)[0]
            out.append((stem, ops.paste_mixed_u8(photo2, sr_packed, sr_meta, regions).cpu().numpy()))
        return out

    def _demo_windows(self, model_list, model_psn, batches, fn, reader, chunk, line_kw=None):
        """demo(tile=True): per batch (names, plan, images_lr) of windows -> (names, one (H, W_b, 3) uint8 array per image, the LR
        reads, the SR reads, (packed, meta), None, None), the reads of an image's windows joined with '|'; packed / meta: the stitched lines
        as ops.stitch_windows_u8 returns them, still on the device.
        line_kw (demo's line_read: {rec, gap}): instead of reading every window, rec.window_rows keeps the frame logits of the LR and
        of the SR windows of every chunk on the device -- a line's windows may span chunks -- and rec.read_lines reads every line
        once per side; the reads are the lines' strings and the sixth item is (lr conf values, sr conf values).  With a lexicon in
        line_kw ({lexicon, penalty}: demo's lexicon with line_read) the SR side's read_lines also reads the line as lexicon words and
        the last item is (the words joined by spaces, the Viterbi scores); None otherwise."""
        from ..utils.confidence import confidence as conf_of
        chunk = max(int(chunk if chunk is not None else self.batch_size), 1)
        for names, plan, images_lr in batches:
            images_lr = images_lr.to(self.device)
            T = images_lr.shape[0]
            srs, reads_lr, reads_sr = [], [], []
            rows_lr, rows_sr = [], []
            for lo in range(0, T, chunk):
                x = images_lr[lo:lo + chunk]
                n = x.shape[0]
                if n == 1:
                    x = torch.cat([x, x], 0)
                label_vecs = self.label_vecs_from_crnn(x) if self.args.arch in ('tatt', 'tpgsr') else None
                sr = self.refine(model_list, model_psn, x, label_vecs, fn)[:n]
                srs.append(sr)
                if line_kw:
                    rows_lr.append(line_kw["rec"].window_rows(x[:n, :3])[0])
                    rows_sr.append(line_kw["rec"].window_rows(sr[:, :3])[0])
                elif reader is not None:
                    reads_lr += [str(s) for s in reader(x[:n, :3])]
                    reads_sr += [str(s) for s in reader(sr[:, :3])]
            packed, meta = ops.stitch_windows_u8(srs[0] if len(srs) == 1 else torch.cat(srs, 0), plan, scale=self.scale_factor)
            flat = packed.cpu().numpy()
            pixels = [flat[off:off + h * w * 3].reshape(h, w, 3) for off, h, w in meta]
            if line_kw:
                lr_w = images_lr.shape[3]
                # (demo's lexicon: the SR side's read_lines also decodes the line as lexicon words, in the same host copy)
                lex_kw = {"lexicon": line_kw["lexicon"], "penalty": line_kw["penalty"]} if line_kw.get("lexicon") is not None else {}
                side = [line_kw["rec"].read_lines(r[0] if len(r) == 1 else torch.cat(r, 0), plan, line_kw["gap"], lr_w, **kw)
                        for r, kw in ((rows_lr, {}), (rows_sr, lex_kw))]
                yield (names, pixels, side[0][0], side[1][0], (packed, meta), (conf_of(*side[0][1:3]), conf_of(*side[1][1:3])),
                       (side[1][4], side[1][5]) if lex_kw else None)
                continue
            preds_lr, preds_sr = [[] for _ in names], [[] for _ in names]
            if reader is not None:
                for (b, _), s_lr, s_sr in zip(plan, reads_lr, reads_sr):
                    preds_lr[b].append(s_lr)
                    preds_sr[b].append(s_sr)
            yield names, pixels, ['|'.join(p) for p in preds_lr], ['|'.join(p) for p in preds_sr], (packed, meta), None, None

    # ------------------------------------------------------------------ training (super_resolution.py:113-278)
    def build_training(self, world_size=1, group=None):
        """models (PGRMs + CMM), frozen PSN, DistillModules, ImageLoss and the flat-bucket clip+Adam / all-reduce trainer.
        self.ema_decay (set by train(ema_decay=...), or by the caller before this call): the trainer also averages the weights."""
        from ..loss.image_loss import ImageLoss
        from ..model.distill_module import DistillModule
        from ..train.optim import Trainer
        models, psn = self.build_models()
        b1, b2 = self.args.stu_iter_b1, self.args.stu_iter_b2
        distill = [DistillModule().to(self.device) for _ in range(b1 + b2 - 2)]
        crit = ImageLoss(gradient=self.args.gradient, loss_weight=[1, 1])
        cfg = self.config.TRAIN
        trainer = Trainer(models + distill, lr=cfg.lr, beta1=cfg.beta1, max_norm=0.25, world_size=world_size, group=group,
                          ema_decay=getattr(self, "ema_decay", None))
        for m in models + distill:
            m.train()
            for p in m.parameters():
                p.requires_grad = True
        # the modules, parameters and buckets built above live as long as the run: out of the garbage collector's generations, or a
        # full collection walks them all in the middle of a step (measured: a 65-85 ms host stall every few dozen steps, a 23 ms step
        # took 44 ms when the launch queue ran dry)
        import gc
        gc.collect()
        gc.freeze()
        return models, psn, distill, crit, trainer

    @staticmethod
    def rotate_pair(images_lr, images_hr, max_deg):
        """Rotation augmentation (super_resolution.py:144-151 / 358-365): one random angle in [-max_deg, max_deg] and one
        aspect-ratio jitter per sample (numpy RNG, like the reference), applied to the LR and HR image alike."""
        import math
        import numpy as np
        from ..utils.util import torch_rotate_img
        bs = images_lr.shape[0]
        angle = np.random.rand(bs) * max_deg * 2 - max_deg
        arc = torch.tensor(angle / 180. * math.pi).float().to(images_lr.device)
        rand_offs = torch.tensor(np.random.rand(bs)).float().to(images_lr.device)
        return torch_rotate_img(images_lr, arc, rand_offs), torch_rotate_img(images_hr, arc, rand_offs)

    def psn_forward(self, psn, images_lr, label_vecs=None):
        """The frozen PSN's image (super_resolution.py:156-169): the arch decides the call signature."""
        with torch.no_grad():
            if self.args.arch in ('tsrn', 'tbsrn', 'tg'):
                return psn(images_lr)
            if self.args.arch == 'tpgsr':
                return psn(images_lr, label_vecs)
            return psn(images_lr, label_vecs)[0]

    def prefetch_psn(self, psn, images_lr, label_vecs=None):
        """The PSN image of the NEXT batch, computed on a lane stream of its own while the current step runs: the PSN is frozen
        (super_resolution.py:56-59), so its output does not depend on the optimisation steps in between, and the step it overlaps
        has single-stream phases (CMM forward / backward, optimizer) with idle CUs.  Returns a handle for train_step(psn_out=...)."""
        dev = images_lr.device
        # one lane per device for the whole process (like the branch and weight-gradient streams): HIP maps streams onto a few hardware
        # queues in creation order, and a second TextSR object's fresh lane landed on a branch stream's queue (bench.py's second
        # training leg in one process: 27.7 vs 27.4 ms)
        lane = _streams.pool(dev)["psn"]
        lane.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(lane):
            out = self.psn_forward(psn, images_lr, label_vecs)
            ev = torch.cuda.Event()
            ev.record(lane)
        return out, ev, images_lr.data_ptr()

    def train_step(self, models, psn, distill, crit, trainer, images_lr, images_hr, label_vecs=None, text_priors=None,
                   text_prior_fn=None, psn_out=None, prefetch=None):
        """One optimisation step = super_resolution.py:140-278 (loss sum / (b1+b2+1), per-model clip 0.25, Adam).
        psn_out: the handle prefetch_psn returned for THIS batch (else the PSN runs here); prefetch = (images_lr, label_vecs) of the
        next batch: its PSN image is started behind this step's branch forward and left in self.psn_prefetched."""
        b1, b2 = self.args.stu_iter_b1, self.args.stu_iter_b2
        share = self.args.sr_share
        trainer.zero_grad()
        if getattr(self.args, "rotate_train", 0):
            images_lr, images_hr = self.rotate_pair(images_lr, images_hr, self.args.rotate_train)
            psn_out = None       # the prefetched image belongs to the unrotated batch
        hr3 = images_hr[:, :3, :]
        if psn_out is not None and psn_out[2] == images_lr.data_ptr():
            images_lr_psn, ev, _ = psn_out
            cur = torch.cuda.current_stream(images_lr.device)
            cur.wait_event(ev)
            images_lr_psn.record_stream(cur)
        else:
            images_lr_psn = self.psn_forward(psn, images_lr, label_vecs)
        br1, br2, part = [], [], [[], []]      # part / dl: the 0-d loss terms of a branch, summed once by _CombineLosses

        def run_branch1():
            cascade = images_lr_psn
            for k in range(b1):
                x_q = text_priors[k] if text_priors is not None else text_prior_fn(cascade.detach(), k)
                sr = models[0 if share else k](x_q, cascade[:, :3, :], br1[:k])
                br1.append(sr)
                cascade = sr
                part[0].append(crit(sr, hr3))

        def run_branch2():
            cascade = images_lr_psn
            for k in range(b1, b1 + b2):
                with torch.no_grad():
                    x_q = ops.to_mask(cascade.detach())      # toMask is not differentiable (PIL round trip in the reference)
                sr = models[0 if share else k](x_q, cascade[:, :3, :], br2[:(k - b2)])
                br2.append(sr)
                cascade = sr
                part[1].append(crit(sr, hr3))

        dl = [[], []]

        def run_distill(branch):
            imgs, off = (br1, 0) if branch == 0 else (br2, b1 - 1)
            feat = imgs[-1]
            for k in range(len(imgs) - 1, 0, -1):
                ld, feat = distill[k - 1 + off](feat, imgs[k - 1])
                dl[branch].append(ld)

        # two HIP streams for the two branches (see refine()); autograd runs each node's backward on its forward's stream and joins
        # the streams at the end of backward().  The step's weight packs are refreshed on the main stream before the fork.
        forked = TRAIN_BRANCH_STREAMS and not share and images_lr.is_cuda and (GRAPH_MULTISTREAM or not torch.cuda.is_current_stream_capturing())
        if forked:
            from ..model import packing
            if packing.ACTIVE is not None:
                packing.ACTIVE.ensure_fresh()
            cur = torch.cuda.current_stream()
            s1, s2 = self._side_streams = side_streams(images_lr.device)
            s1.wait_stream(cur)
            s2.wait_stream(cur)
            # the distillation chain of a branch (super_resolution.py:219-236) needs that branch's images only: it stays on the
            # branch's stream BEHIND the event the CMM waits for, so it -- and, since autograd runs a node's backward on its forward's
            # stream, its backward -- overlaps the CMM's single-stream forward / backward instead of preceding it
            with torch.cuda.stream(s1):
                run_branch1()
                e1 = torch.cuda.Event()
                e1.record(s1)
                if DISTILL_ON_BRANCH:
                    run_distill(0)
            with torch.cuda.stream(s2):
                run_branch2()
                e2 = torch.cuda.Event()
                e2.record(s2)
                if DISTILL_ON_BRANCH:
                    run_distill(1)
            cur.wait_event(e1)
            cur.wait_event(e2)
            for t_ in br1 + br2:
                t_.record_stream(cur)
        else:
            run_branch1()
            run_branch2()
        self.psn_prefetched = None
        if prefetch is not None and not getattr(self.args, "rotate_train", 0) and not torch.cuda.is_current_stream_capturing():
            self.psn_prefetched = self.prefetch_psn(psn, *prefetch)      # overlaps the CMM forward, the backward and the optimizer
        if not (forked and DISTILL_ON_BRANCH):
            run_distill(0)
            run_distill(1)
        sr = models[-1](br1[-1], br2[-1])
        lc = crit(sr, hr3)
        if forked and DISTILL_ON_BRANCH:
            cur.wait_stream(s1)
            cur.wait_stream(s2)
        terms = part[0] + part[1] + dl[0] + dl[1] + [lc]
        if forked:
            for t_ in terms[:-1]:
                t_.record_stream(cur)
        # loss = (sum_k 100 ImageLoss_k + sum_j 100 distill_j + 100 ImageLoss_cmm) / (b1 + b2 + 1)   (super_resolution.py:205-262)
        if os.environ.get("DPMN_COMBINE_LOSSES", "1") != "0":
            loss = _CombineLosses.apply(b1 + b2 + 1, *terms)
        else:
            loss = 0
            for t_ in terms:
                loss = loss + t_.mean() * 100
            loss = loss / (b1 + b2 + 1)
        if hasattr(trainer, "arm_early_step"):
            trainer.arm_early_step()      # trainer.step() follows: a model's clip + Adam may run as soon as its backward has finished
        try:
            loss.backward()
            if forked:
                # the PGRMs' backward kernels ran on the side streams and wrote the gradient arena directly (no AccumulateGrad node the
                # autograd engine would join on): the optimizer kernels on this stream must wait for them explicitly
                cur = torch.cuda.current_stream()
                cur.wait_stream(self._side_streams[0])
                cur.wait_stream(self._side_streams[1])
            trainer.step()
        finally:
            # the promise made by arm_early_step() ends with this call whatever happened: if step() was not reached the gradients a
            # backward left on a side stream are joined here, so a caller that inspects p.grad or retries sees complete buffers
            if hasattr(trainer, "disarm"):
                trainer.disarm()
        return loss.detach()

    def graphed_train_step(self, models, psn, distill, crit, trainer, images_lr, images_hr, label_vecs=None, text_priors=None,
                           warmup=3):
        """hipGraph capture of one whole training step (~2000 launches): returns run(images_lr, images_hr, label_vecs,
        text_priors) -> loss that copies the batch into the captured step's static inputs and replays the graph.
        Static shapes, precomputed text priors, single process (the RCCL exchange is left to the eager path)."""
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError("dpmn_amd: graphed_train_step is single-process; multi-GPU runs use train_step")
        assert text_priors is not None, "graph capture needs the text priors as inputs"
        for m in models:
            dp = getattr(m, "drop_probs", None)
            if dp is not None and (dp[0] > 0 or dp[1] > 0 or max(dp[2]) > 0):
                raise RuntimeError("dpmn_amd: graphed_train_step would freeze the Dropout / DropPath seeds (kernel arguments) into "
                                   "the captured graph and replay the same masks every step; train with train_step, or zero rates")
        trainer.device_step_counter()
        st = dict(lr=images_lr.clone(), hr=images_hr.clone(), lv=None if label_vecs is None else label_vecs.clone(),
                  tp=[t.clone() for t in text_priors])
        call = lambda: self.train_step(models, psn, distill, crit, trainer, st["lr"], st["hr"], st["lv"], text_priors=st["tp"])
        # the warm-up steps and the capture pass (which only records) must not train: snapshot everything a step mutates
        # (parameters, Adam moments and step count, BatchNorm running statistics) and put it back afterwards
        snap = trainer.state_snapshot()
        bufs = [b for m in models + distill for b in m.buffers()]
        buf_snap = [b.clone() for b in bufs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):          # allocator pools, workspaces and kernel attributes settle before capture
                call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = call()
        trainer.state_restore(snap)
        for b, s_ in zip(bufs, buf_snap):
            b.copy_(s_)

        def run(images_lr, images_hr, label_vecs=None, text_priors=None):
            st["lr"].copy_(images_lr)
            st["hr"].copy_(images_hr)
            if label_vecs is not None:
                st["lv"].copy_(label_vecs)
            if text_priors is not None:
                for d, s_ in zip(st["tp"], text_priors):
                    d.copy_(s_)
            graph.replay()
            # the replayed optimizer kernels rewrote the parameters through raw pointers: eval-mode weight packs (CMM) and the
            # PGRMs' LayerNorm-folded attention weights cached before this step are stale now (trainer.step() in Python, which
            # drops them on the eager path, ran only while the graph was captured)
            trainer.invalidate_packs()
            return loss
        run.graph = graph
        return run

    def train(self, loader=None, steps=None, val_loader=None, rec=None, epochs=None, sampler=None, display=False, state_path=None,
              ema_decay=None, train_words=None):
        """Training loop (super_resolution.py:125-337) over (images_hr, images_lr, label_vecs) batches (synthetic ones, or the
        TextZoom reader of dataset/textzoom.py through main.py).
        loader: a callable `loader(epoch) -> iterable` (a fresh pass per epoch), a re-iterable (list, DataLoader-like: walked
        once per epoch for `epochs` / config.TRAIN.epochs epochs, `for epoch in range(cfg.epochs)` of the reference), or a
        one-shot iterator (a single epoch).  sampler: a DistributedSampler whose set_epoch is called per epoch.
        Bookkeeping as in the reference: iters = len(loader) * epoch + j + 1 counted globally, display every displayInterval,
        eval + best-model checkpoint every VAL.valInterval when a val_loader is given (best = recognition accuracy when `rec`
        computes one, else PSNR), checkpoint.pth every saveInterval and at the end, epoch written to checkpoints and log.csv.
        Rank 0 writes the files; under ZeRO-1 every save waits for the step's parameter all-gather first (trainer.sync_params:
        the gather runs asynchronously on RCCL's stream, a state_dict clone before it lands would tear the checkpoint).
        display=True: every evaluation pass writes its comparison images (eval(display=True), index = epoch; rank 0 only).
        state_path (main.py --train_state): ONE file that lets an interrupted run continue bit for bit (interfaces/base.py "training
        state").  If it exists the run continues from it -- weights, BatchNorm statistics, Adam state, bookkeeping, the
        random streams, the position inside the epoch -- else the run starts fresh; rank 0 rewrites it (atomically) after every
        iteration that saved a checkpoint and at the end of the run.  `it` goes on counting and `steps` stays a total.  Without it
        nothing is read or written beyond the files above.
        ema_decay (main.py --ema, 0 < d < 1): the trainer keeps an exponential moving average of the weights, e = d * e + (1 - d) * p
        after every step, started as a copy of the weights the models are built with (BasicSR's ema_decay).  Every validation pass
        runs under the averaged weights (Trainer.ema_weights(); the BatchNorm statistics stay the live ones) and the best-model
        checkpoints written from it hold them -- they are what was scored; checkpoint.pth keeps the live weights, the state file
        carries the average, and a state only continues a run with the same setting.
        train_words (main.py --train_words): the setting of a run whose HR images are rendered from a word list
        (utils.render.words_setting: crc32 of the list, font names, epoch size and, with --train_words_fx, the kinds, the probability
        and the background pool's crc32; the loader itself comes from
        get_train_data(train_words=...)).  It only goes into the state's fingerprint: a state continues a run with the same setting."""
        dist = torch.distributed
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.ema_decay = ema_decay
        fingerprint = base.state_fingerprint(self.args, self.config, ema=ema_decay, train_words=train_words)
        models, psn, distill, crit, trainer = self.build_training(world)
        if getattr(self, "rank_seed", None) is not None:      # models are built (and broadcast): now diverge the per-rank RNG
            from ..utils.util import set_seed
            set_seed(self.rank_seed)
        fn = self.default_text_prior()
        if loader is None:
            raise RuntimeError("dpmn_amd: pass a loader of (images_hr, images_lr, label_vecs) batches")
        cfg = self.config.TRAIN
        val_int = getattr(getattr(cfg, "VAL", None), "valInterval", None) or 80
        log_path = os.path.join(getattr(cfg, "ckpt_dir", None) or ".", "log.csv")
        best, best_info, converge = None, {}, []
        best_hist = {}         # best_history_acc[data_name] of the reference (super_resolution.py:299-313)
        # validation subsets: {data_name: loader | callable -> loader}; a bare loader / callable is one subset named "val"
        if val_loader is None:
            val_sets = []
        elif isinstance(val_loader, dict):
            val_sets = list(val_loader.items())
        else:
            val_sets = [("val", val_loader)]
        if callable(loader):
            passes = loader
            n_epochs = epochs if epochs is not None else int(getattr(cfg, "epochs", 1) or 1)
        elif hasattr(loader, "__next__"):      # a generator can be walked once
            passes = lambda _e: loader
            n_epochs = 1
        else:
            passes = lambda _e: loader
            n_epochs = epochs if epochs is not None else int(getattr(cfg, "epochs", 1) or 1)

        def save(epoch, it, is_best, metric="sum"):
            nonlocal dirty
            dirty = True
            if rank == 0:
                self.save_checkpoint(models, epoch, it, dict(best_hist, score=best), best_info, is_best, converge, None, metric=metric, trainer=trainer)

        def log_row(row):
            if rank == 0:
                os.makedirs(os.path.dirname(log_path) or ".", exist_ok=True)
                with open(log_path, "a+", newline="") as out:
                    csv.writer(out).writerow(row)

        it, epoch, saved_at = 0, 0, -1
        first_epoch, done, state, rng_epoch, dirty, loss, wrote_at = 0, 0, None, None, False, None, -1
        if state_path is not None and os.path.isfile(state_path):
            # continue: fingerprint first, then weights + BatchNorm statistics (written through the state_dicts: views of the trainer's
            # parameter arena), Adam state, bookkeeping; the random streams follow in the epoch loop
            state = base.read_train_state(state_path, fingerprint)
            for m_, sd in zip(models + distill, state["models"] + state["distill"]):
                m_.load_state_dict(sd)
            trainer.load_state_dict(state["trainer"])
            lp = state["loop"]
            it, first_epoch, done, saved_at = lp["it"], lp["epoch"], lp["done"], lp["saved_at"]
            best, best_hist, best_info, converge = lp["best"], dict(lp["best_hist"]), lp["best_info"], list(lp["converge"])
            epoch, wrote_at = first_epoch, it
            if rank == 0 and lp["log_rows"] is not None and os.path.isfile(log_path):
                with open(log_path, newline="") as f:      # rows of evaluations after the state was written: they will be written again
                    rows = f.readlines()
                if len(rows) > lp["log_rows"]:
                    with open(log_path, "w", newline="") as f:
                        f.writelines(rows[:lp["log_rows"]])
            if rank == 0:
                print("continuing from %s: epoch %d, iter %d" % (state_path, first_epoch, it))
            # the frozen CRNN behind TATT's label_vecs is built on first use, and building a module draws its initial weights from
            # torch's generator: in the run that wrote the state that happened before its first step, so here it has to happen before
            # the random streams are restored, not after (a shuffling loader's next permutation comes from that generator)
            if self.args.arch in ('tatt', 'tpgsr') and getattr(self, "_crnn_psn", None) is None and os.path.isfile(self._psn_crnn_path() or ""):
                from ..model.crnn import load_crnn
                self._crnn_psn = load_crnn(self._psn_crnn_path(), self.device)

        def restore_rng(which):
            per_rank = state["rng"]
            if rank < len(per_rank):
                base.rng_restore(per_rank[rank][which], self.device)
            elif which == "now":      # (a larger world than the one that wrote the state: no exact continuation is promised)
                from ..utils.util import set_seed
                seed = (self.rank_seed if getattr(self, "rank_seed", None) is not None else rank) + 7919 * it
                print("rank %d: no random-number state in %s (written by %d ranks), re-seeded with %d" % (rank, state_path, len(per_rank), seed))
                set_seed(seed)

        def write_state():
            """Collective: the trainer's ZeRO-1 shards and every rank's random-number state are gathered; rank 0 writes."""
            tsd = trainer.state_dict()
            rng = {"epoch_start": rng_epoch, "now": base.rng_capture(self.device)}
            per_rank = [rng]
            if world > 1:
                per_rank = [None] * world
                dist.all_gather_object(per_rank, rng)
            if rank != 0:
                return
            log_rows = None
            if os.path.isfile(log_path):
                with open(log_path, newline="") as f:
                    log_rows = len(f.readlines())
            cpu_sd = lambda m_: {k: v.detach().cpu() for k, v in m_.state_dict().items()}
            base.write_train_state(state_path, {
                "version": base.TRAIN_STATE_VERSION, "fingerprint": fingerprint, "world": world,
                "models": [cpu_sd(m_) for m_ in models], "distill": [cpu_sd(m_) for m_ in distill], "trainer": tsd, "rng": per_rank,
                "loop": dict(loop_state(), log_rows=log_rows)})

        def loop_state():
            return {"epoch": epoch, "it": it, "done": done, "saved_at": saved_at, "best": best, "best_hist": dict(best_hist),
                    "best_info": best_info, "converge": list(converge)}

        for epoch in range(first_epoch, n_epochs):
            if sampler is not None and hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            resumed = state is not None and epoch == first_epoch
            if resumed:
                restore_rng("epoch_start")      # a shuffling loader draws its permutation when its iterator is made: the same one again
            if state_path is not None:
                rng_epoch = base.rng_capture(self.device)
            done = 0
            def on_device(data):
                hr, lr = data[0].to(self.device), data[1].to(self.device)
                lv = data[2].to(self.device) if len(data) > 2 and data[2] is not None else None
                if lv is None and self.args.arch in ('tatt', 'tpgsr'):
                    lv = self.label_vecs_from_crnn(lr)
                return hr, lr, lv
            batches = iter(passes(epoch))
            if resumed:
                while done < lp["done"] and next(batches, None) is not None:      # the batches this epoch already trained on
                    done += 1
                restore_rng("now")
                if steps is not None and it >= steps:
                    break
            nxt = next(batches, None)
            nxt = on_device(nxt) if nxt is not None else None
            handle = None
            while nxt is not None:
                hr, lr, lv = nxt
                # one batch of look-ahead (its frozen-PSN image is computed during this step) -- fetched before the step is issued only
                # when the prefetch can be used: not past the last requested step (a one-shot loader would lose the batch), not with
                # rotate_train (the PSN sees the rotated batch, which does not exist yet)
                ahead = (steps is None or it + 1 < steps) and not getattr(self.args, "rotate_train", 0)
                nxt = next(batches, None) if ahead else None
                nxt = on_device(nxt) if nxt is not None else None
                loss = self.train_step(models, psn, distill, crit, trainer, lr, hr, lv, text_prior_fn=fn, psn_out=handle,
                                       prefetch=None if nxt is None else (nxt[1], nxt[2]))
                handle = self.psn_prefetched
                if not ahead and not (steps is not None and it + 1 >= steps):      # no look-ahead: fetch the next batch after the step was issued
                    nxt = next(batches, None)
                    nxt = on_device(nxt) if nxt is not None else None
                it += 1
                done += 1
                if it % cfg.displayInterval == 0 and rank == 0:
                    print('Epoch: [%d] iter %d | Loss: %f' % (epoch, it, float(loss)))
                if val_sets and it % val_int == 0:
                    # super_resolution.py:293-330: every validation subset on its own -- a log.csv row and a best-so-far checkpoint
                    # per data_name -- and the best model overall by the SUM of the subsets' scores (score = recognition accuracy
                    # when `rec` computes one, as in the reference; PSNR otherwise, e.g. without --rec crnn)
                    trainer.sync_params()
                    # with the average on, the pass scores the averaged weights, and the best-model files written inside it hold them
                    with (trainer.ema_weights() if ema_decay is not None else contextlib.nullcontext()):
                        current, psnr_d, ssim_d = {}, {}, {}
                        for data_name, vl in val_sets:
                            md = self.eval(models, vl() if callable(vl) else vl, epoch, rec=rec, model_psn=psn, text_prior_fn=fn,
                                           display=display and rank == 0)
                            converge.append({'iterator': it, 'acc': md['accuracy'], 'psnr': md['psnr_avg'], 'ssim': md['ssim_avg']})
                            score = md['accuracy'] if md['accuracy'] is not None else md['psnr_avg']
                            current[data_name], psnr_d[data_name], ssim_d[data_name] = float(score), md['psnr_avg'], md['ssim_avg']
                            new_best = data_name not in best_hist or score > best_hist[data_name]
                            if new_best:
                                best_hist[data_name] = float(score)
                                best_hist['epoch'] = epoch
                                best_info = {'accuracy': md['accuracy'], 'psnr': md['psnr_avg'], 'ssim': md['ssim_avg']}
                                if len(val_sets) > 1:
                                    save(epoch, it, True, data_name)
                            log_row([epoch, data_name, md['accuracy'], md['psnr_avg'], md['ssim_avg']] + (["best_%s" % data_name] if new_best else []))
                        for m_ in models + distill:
                            m_.train()
                        total = sum(current.values())
                        if best is None or total > best:
                            best = total
                            best_info = {'accuracy': dict(current, epoch=epoch), 'psnr': psnr_d, 'ssim': ssim_d}
                            save(epoch, it, True)
                            log_row([epoch, "", "", "", "", "", "best_sum"])
                if it % cfg.saveInterval == 0:
                    save(epoch, it, False)
                    saved_at = it
                if (state_path is not None and (it % cfg.saveInterval == 0 or (val_sets and it % val_int == 0))
                        and not (steps is not None and it >= steps)):      # (the last requested step: the write at the end of the run follows)
                    # once per iteration, after ALL of its bookkeeping: the file never holds half an evaluation.  Whether a "best"
                    # save happened is rank 0's call (BatchNorm statistics, hence scores, are per rank) and the write is a collective
                    flag = [dirty]
                    if world > 1:
                        dist.broadcast_object_list(flag, src=0)
                    if flag[0]:
                        write_state()
                        wrote_at = it
                    dirty = False
                if steps is not None and it >= steps:
                    break
            if steps is not None and it >= steps:
                break
        final_save = saved_at != it
        if final_save:
            save(epoch, it, False)
            saved_at = it
        if state_path is not None and rng_epoch is not None and (final_save or wrote_at != it):      # (rng_epoch None: no epoch was entered)
            write_state()
        trainer.sync_params()
        self.trainer = trainer
        self.last_loss, self.loop_state = loss, loop_state()      # (the last step's loss, None if no step ran; the bookkeeping as a state holds it)
        return models, distill

    def label_vecs_from_crnn(self, images_lr):
        """--arch tatt on real data (super_resolution.py:165-169): label_vecs = softmax of the frozen CRNN's logits on the LR
        image, reshaped (T, B, 37) -> (B, 37, 1, T).  The CRNN is loaded from <resume>/recognizer_best_crnn.pth (line 92)."""
        crnn = getattr(self, "_crnn_psn", None)
        if crnn is None:
            from ..model.crnn import load_crnn
            crnn = self._crnn_psn = load_crnn(self._psn_crnn_path(), self.device)
        return crnn.label_vecs(images_lr[:, :3])

    def _psn_crnn_path(self):
        return os.path.join(self.resume, "recognizer_best_crnn.pth") if self.resume and os.path.isdir(self.resume) else None

    def test(self, loader=None, rec=None, display=False, lexicon=None, beam=None):
        """super_resolution.py:515-775: PGRMs from model_best_{k}.pth, CMM from model_best_cmm.pth, PSN from model_{arch}.pth
        under --resume (all required: there is no evaluation of untrained weights).  display=True: the comparison images of the
        last batch under <vis_dir>/0/ and those of every wrongly read image under <vis_dir>/display/ (their number: 'visualized').
        lexicon: eval's (an ops.Lexicon: the dict gains 'accuracy_lexicon'); beam: eval's (the dict gains 'accuracy_lm')."""
        models, psn = self.build_models(testing=True)
        if loader is None:
            raise RuntimeError("dpmn_amd: pass a loader of (images_hr, images_lr, label_vecs) batches: "
                               "dataset.textzoom.sr_batches(self.get_test_data(dir)[1], device) or dpmn_amd.utils.synth.synth_batch")
        if lexicon is not None or beam is not None:
            more = dict(({"lexicon": lexicon} if lexicon is not None else {}), **({"beam": beam} if beam is not None else {}))
            return self.eval(models, loader, 0, rec=rec, model_psn=psn, display=display, display_failures=display, **more)
        return self.eval(models, loader, 0, rec=rec, model_psn=psn, display=display, display_failures=display)
