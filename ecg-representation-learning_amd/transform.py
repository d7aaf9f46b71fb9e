"""
Input transforms of the reference data pipeline, FUSED into the patch-embed load.

Reference: `ecg_transformer/preprocess/transform.py` -- `Normalize` (:18-35), `TimeEndPad` (:140-154), `TimeOut` (:175-185) --
composed per record on the host in `get_ptbxl_dataset` (`preprocess/ptb_dataset.py:132-149`: Normalize, TimeEndPad(patch_size),
and TimeOut for the training split only).  Here the raw `(B, 12, L_raw)` batch goes to the device as is and the three
transforms are applied inside `ecgvit_patch_gather_transform` while the samples stream through LDS: no extra read+write of
the input tensor, no per-record numpy work on the host.  Only the TimeOut span is drawn on the host (two int32 per record), with
the same torch RNG calls the reference makes, so a seeded run masks the same spans.

`per_record=True`: the records need not share a raw length.  `lengths[b]` is then record b's RAW sample count l_b (any integer >= 1), in a
padded `(B, 12, W)` batch (W >= max l_b; samples at or past l_b are never read) or a ragged `(12, S_raw)` one (the raw records
concatenated).  Record b is transformed as the reference transforms it alone -- normalised, zero-padded in normalised space to
`padded_length(l_b)`, TimeOut drawn on that padded length (`draw_timeout_records`) -- inside `ecgvit_patch_gather_transform_varlen`, and
counts `padded_length(l_b) / patch_size` patches from there on.  Without `per_record` (the default) per-record lengths and ragged batches
are refused as before: the rectangular kernel pads every record to one length.
"""
import torch


class FusedInputTransform:
    def __init__(self, mean, std, patch_size, timeout=False, timeout_scale=(0.0, 0.5), per_record=False):
        mean = torch.as_tensor(mean, dtype=torch.float32)
        std = torch.as_tensor(std, dtype=torch.float32)
        assert mean.numel() == 12 and std.numel() == 12   # transform.py:26
        self.mean, self.inv_std = mean.contiguous(), (1.0 / std).contiguous()
        self.k = int(patch_size)
        self.timeout = bool(timeout)
        self.per_record = bool(per_record)
        self.sampler = torch.distributions.Uniform(low=timeout_scale[0], high=timeout_scale[1])   # transform.py:178
        self._dev = None

    def padded_length(self, l_raw: int) -> int:
        """TimeEndPad: n_pad = k - (l % k)  -- a FULL extra patch when l is already a multiple of k (transform.py:150)"""
        return l_raw + (self.k - (l_raw % self.k))

    def draw_timeout(self, batch: int, l_pad: int, device):
        """per record: r ~ U(lo, hi); l_crop = round(r * L); start = randint(L - l_crop)  (transform.py:180-183), as int32 tensors"""
        starts, lens = [], []
        for _ in range(batch):
            r = self.sampler.sample().item()
            l_crop = round(r * l_pad)
            start = torch.randint(high=l_pad - l_crop, size=(1,)).item()
            starts.append(start)
            lens.append(l_crop)
        return (torch.tensor(starts, dtype=torch.int32, device=device), torch.tensor(lens, dtype=torch.int32, device=device))

    def draw_timeout_records(self, padded_lengths):
        """`draw_timeout` for records of unequal length: per record, in batch order, the reference's two RNG calls on that record's own padded
        length (transform.py:180-183) -> (2, B) int32 HOST tensor [starts; lengths] (the engine stages it through pinned memory).  Drawing a
        batch range by range, in order, consumes the generator exactly as drawing it whole."""
        out = torch.empty(2, len(padded_lengths), dtype=torch.int32)
        for b, l_pad in enumerate(int(v) for v in padded_lengths):
            r = self.sampler.sample().item()
            l_crop = round(r * l_pad)
            out[0, b] = torch.randint(high=l_pad - l_crop, size=(1,)).item()
            out[1, b] = l_crop
        return out

    def device_stats(self, device):
        if self._dev is None or self._dev[0].device != device:
            self._dev = (self.mean.to(device), self.inv_std.to(device))
        return self._dev
