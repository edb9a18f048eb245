"""A word list as the HR images of a TRAINING set (main.py --train_words): nothing is read from disk but the list, and every sample
knows its label.  The loader's workers render nothing and never open the GPU: an item is a word index, the collate function
(dataset/textzoom.py alignCollate_realWTLAMask(render=...)) leaves the image positions empty, and `sr_batches` draws the words and the
render parameters of a batch in the main process (utils/render.py draw_render, from the per-pass keyed stream that --train_state
restores), renders the batch on the GPU (ops.render_words_u8) and degrades it like a batch of --train_hr_dir.  With --train_words_fx the
collate function also carries the utils.render.RenderFx (kinds, probability, background pool): the draws are then draw_render_fx's
and the render is ops.render_words_fx_u8; with --train_words_warp it carries the utils.render.RenderWarp too (kinds, probability,
magnitudes): draw_render_warp's draws and ops.render_words_warp_u8.  The workers still see word indices only.  The set has no end of its
own: its length is the number of samples that counts as one epoch, and what a DistributedSampler shards."""
import torch


class WordsHR(torch.utils.data.Dataset):
    """Items (None, None, None, None, word) in the layout of folder.FolderHR's -- the image positions are empty.  The word of item i is
    words[i % len(words)]: a placeholder that only keeps the collate function's label tensors well-formed; the words that are rendered,
    and the labels `sr_batches` yields, are drawn per batch."""

    def __init__(self, words, epoch_size=10000):
        super().__init__()
        self.words = list(words)
        self.epoch_size = int(epoch_size)
        if not self.words:
            raise ValueError("WordsHR: an empty word list")
        if self.epoch_size < 1:
            raise ValueError("WordsHR: the epoch size must be positive, got %d" % self.epoch_size)

    def __len__(self):
        return self.epoch_size

    def __getitem__(self, index):
        if not 0 <= index < self.epoch_size:
            raise IndexError(index)
        return None, None, None, None, self.words[index % len(self.words)]
