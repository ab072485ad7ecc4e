#!/usr/bin/env python
"""Synthesis driver with the reference's command line (reference predict_mel.py:2-15,58-74).

Usage: predict_mel.py --source-data-root=<dir> --target-data-root=<dir> --checkpoint-dir=<dir> --output-dir=<dir>
                      --selected-list-dir=<dir> [--checkpoint=<file>] [--selected-list-filename=<name>]
                      [--hparams=<a=b>] [--hparam-json-file=<path>] [--batch-size=<N>] [--stop-per-utterance]
                      [--wav] [--griffin-lim-iters=<N>] [--griffin-lim-power=<P>] [--inversion=pinv|nnls] [--nnls-iters=<N>]

For every key of the list: free-running decode (batch size 1) from `model-<step>.pt`, output `<key>.mfbsp` (raw
little-endian float32 [T, num_mels]; the PostNetV2 output when `use_postnet_v2`, models/models.py:440-462), `<key>.alignment.npz` + `<key>.png` (the
two alignment histories laid out [T_memory, T_query] as in the reference's predictions) and `<key>.tfrecord` (the
reference's prediction record, utils/tfrecord.py:135-152).  `use_forced_alignment_mode=True` (models/models.py:387-428):
pass 1 is the validation decode fed with the GROUND-TRUTH mel (needs --target-data-root), pass 2 feeds its own outputs
back while both attention mechanisms return pass 1's alignments.  `--batch-size N` (forced-alignment mode only) decodes N
utterances per pass; `--batch-size N --stop-per-utterance` decodes N free-running utterances at once, each ending at its own stop
token.  `--wav` adds `<key>.wav`: Griffin-Lim phase reconstruction of the de-normalised mel (csrc/griffin_lim.hip); with
`--inversion nnls` its magnitudes come from the non-negative mel inversion (csrc/mel_nnls.hip) instead of the floored pseudo-inverse.
Usage: see --help"""
import argparse
import glob
import os
import sys

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source-data-root", required=True)
    ap.add_argument("--target-data-root", default=None)
    ap.add_argument("--checkpoint-dir", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--selected-list-dir", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--selected-list-filename", default="test.csv")
    ap.add_argument("--hparams", default="")
    ap.add_argument("--hparam-json-file", default=None)
    ap.add_argument("--batch-size", type=int, default=1, metavar="N",
                    help="utterances per decode, 1 .. 16 (default 1, the reference's).  N > 1 needs use_forced_alignment_mode=True: both "
                         "passes then decode N utterances at once and every prediction is cut to its own utterance's lengths.  The "
                         "values are those of the model AT THAT BATCH: the padding symbols of the shorter utterances reach the "
                         "encoder's convolutions exactly as in training, so they are not bit-equal to a batch-size-1 run")
    ap.add_argument("--stop-per-utterance", action="store_true",
                    help="free-running synthesis of --batch-size 2 .. 16 utterances per decode: every utterance ends at its own stop "
                         "token and its prediction is cut there (the decode runs until the last one has ended, at most max_iters "
                         "steps).  As with the forced batches, the values are those of the model at that batch.  Not with "
                         "use_forced_alignment_mode=True, whose passes run the target's number of steps")
    ap.add_argument("--wav", action="store_true",
                    help="write <key>.wav next to every <key>.mfbsp: Griffin-Lim phase reconstruction of the de-normalised mel (16-bit "
                         "PCM at hparams.sample_rate, peak 0.95) - a quick listen, not a vocoder; mel_to_wav.py does the same afterwards")
    ap.add_argument("--griffin-lim-iters", type=int, default=60, metavar="N", help="Griffin-Lim iterations of --wav (default 60)")
    ap.add_argument("--griffin-lim-power", type=float, default=1.0, metavar="P",
                    help="exponent on the linear magnitudes of --wav (default 1.0)")
    ap.add_argument("--inversion", choices=("pinv", "nnls"), default="pinv",
                    help="mel -> linear magnitudes of --wav: the floored pseudo-inverse (default) or the non-negative solve that starts "
                         "from it")
    ap.add_argument("--nnls-iters", type=int, default=64, metavar="N", help="iterations of --inversion nnls (default 64)")
    a = ap.parse_args(argv)
    if not 0 <= a.nnls_iters <= 1024:
        raise SystemExit("--nnls-iters: 0 .. 1024")
    if not 1 <= a.batch_size <= 16:
        raise SystemExit("--batch-size: 1 .. 16")
    if a.griffin_lim_iters < 0:
        raise SystemExit("--griffin-lim-iters: >= 0")

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.datasets.dataset_factory import dataset_factory
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    from satt_amd.utils import tfrecord
    from satt_amd.utils.summary import plot_alignments
    from train import load_key_list

    if a.hparam_json_file:
        hparams.parse_json(open(a.hparam_json_file).read())
    hparams.parse(a.hparams)
    if hparams.use_forced_alignment_mode and not a.target_data_root:
        raise SystemExit("use_forced_alignment_mode aligns to the reference audio: --target-data-root is required")
    if a.stop_per_utterance and hparams.use_forced_alignment_mode:
        raise SystemExit("--stop-per-utterance is the stop rule of free-running synthesis: use_forced_alignment_mode=True decodes the "
                         "target's number of steps")
    if a.batch_size > 1 and not hparams.use_forced_alignment_mode and not a.stop_per_utterance:
        # (the reference's stop rule of a batch fires only when EVERY sample is above the threshold at the same step; where to cut
        #  each sample of a free-running batch is decided by --stop-per-utterance alone)
        raise SystemExit("--batch-size > 1 needs use_forced_alignment_mode=True: a free-running batch has no per-utterance end "
                         "(or --stop-per-utterance, which gives it one)")
    # reference predict_mel.py:40-57: estimator = tacotron_model_factory(hparams, checkpoint_dir, run_config);
    # estimator.predict(input_fn, checkpoint_path=...)
    audio = None
    if a.wav:
        if not np.any(np.asarray(hparams.stddev_mel_level_db, np.float64)):
            raise SystemExit("--wav de-normalises the prediction: average_mel_level_db / stddev_mel_level_db are unset, pass the "
                             "hparams.json that the preprocessing run wrote")
        from satt_amd.utils.audio import Audio
        audio = Audio(hparams, backend="hip")
    model = tacotron_model_factory(hparams, None, device="cuda")
    ck = a.checkpoint or max(glob.glob(os.path.join(a.checkpoint_dir, "model-*.pt")),
                             key=lambda p: int(p.rsplit("-", 1)[1][:-3]))
    model.restore(ck)
    os.makedirs(a.output_dir, exist_ok=True)
    keys = load_key_list(a.selected_list_filename, a.selected_list_dir)
    src = [os.path.join(a.source_data_root, "%s.%s" % (k, hparams.source_file_extension)) for k in keys]
    have_target = bool(a.target_data_root) and all(
        os.path.exists(os.path.join(a.target_data_root, "%s.%s" % (k, hparams.target_file_extension))) for k in keys)

    def input_fn():
        if have_target:
            tgt = [os.path.join(a.target_data_root, "%s.%s" % (k, hparams.target_file_extension)) for k in keys]
            # batch size 1 unless --batch-size, targets merged into the source side (reference predict_mel.py:46-50)
            return dataset_factory(src, tgt, hparams).prepare_and_zip().group_by_batch(batch_size=a.batch_size) \
                .merge_target_to_source()
        # no targets: the dataset's own source padding (the pad values, unknown-id mapping and missing-field error of group_by_batch)
        from satt_amd.datasets.ljspeech import source_batches
        return source_batches(src, hparams, a.batch_size)

    for p in model.predict(input_fn, stop_each=a.stop_per_utterance):
        key = p["key"]
        mel = (p["mel_postnet"] if "mel_postnet" in p else p["mel"]).astype("<f4")
        assert mel.shape[1] == hparams.num_mels
        mel.tofile(os.path.join(a.output_dir, "%s.%s" % (key, hparams.predicted_mel_extension)))
        if audio is not None:
            audio.save_wav_pcm16(audio.inv_melspectrogram(audio.denormalize_mel(mel).T, iters=a.griffin_lim_iters,
                                                          power=a.griffin_lim_power, inversion=a.inversion, nnls_iters=a.nnls_iters),
                                 os.path.join(a.output_dir, "%s.wav" % key))
        # [T_memory, T_query]; the single-source baseline model has one history (reference models/models.py:196-212)
        aligns = [p[k] for k in ("alignment", "alignment2") if k in p]
        np.savez(os.path.join(a.output_dir, "%s.alignment.npz" % key), **{k: p[k] for k in ("alignment", "alignment2") if k in p})
        plot_alignments(os.path.join(a.output_dir, "%s.png" % key), aligns)
        gt = None
        if a.target_data_root:          # the RAW reference mel (un-normalised), as the reference's record holds it
            from satt_amd.datasets.ljspeech import decode_target_record
            tf_ = os.path.join(a.target_data_root, "%s.%s" % (key, hparams.target_file_extension))
            if os.path.exists(tf_):
                gt = decode_target_record(next(tfrecord.read_records(tf_)))["mel"]
        tfrecord.write_prediction_result(p["id"], key, aligns, mel, gt, p["text"] or "", p["source"], p.get("accent_type"),
                                         os.path.join(a.output_dir, "%s.tfrecord" % key))
        print("%s: %d frames" % (key, mel.shape[0]))


if __name__ == "__main__":
    main()
