"""`composer train | evaluate | generate | score | novelty | make-config | summary` for the Transformer hot path.

Mirrors the commands, arguments and defaults of the reference's composer/cli.py (train :516-589, evaluate :591-615,
generate :617-680, make-config :69-78, summary :424-440) with the TensorFlow model replaced by the HIP one.  Out of
scope: the MusicRNN model type, MIDI preprocessing/synthesis.  `export-dataset` (:346-380) and
`.tfrecord` dataset paths (:232-268) go through composer_amd.tfrecord.
Documented divergences: `--temperature 0` means greedy argmax (the reference divides by the temperature, cli.py:671);
besides the reference's MIDI prompt (`--prompt`, read by composer_amd.midi instead of pretty_midi) a prompt can be given
as event ids (`--prompt-ids` / `--prompt-data`), and an output path ending in `.data` gets event ids instead of a MIDI
file; `--decode-mode` selects the literal loop of cli.py:663-676 or a real KV cache.  `score` (not in the reference) prints the
per-event likelihood of MIDI / `.data` files under a restored model; `generate --keep-best` ranks the samples by it.  `novelty` (not in
the reference either) finds the longest verbatim match of every event of such files in a dataset split; `generate --novelty-against`
prints it for the samples."""
import collections
import datetime
import json
import logging
import math
import os
import shutil
import sys
from enum import Enum, unique
from pathlib import Path

import click
import numpy as np

from . import config as cfgmod
from . import dataset as ds
from . import tfrecord
from .augment import check_augment_options
from .transformer import ModelSaveFrequencyMode, Transformer, check_eval_options, check_train_options


@unique
class ModelType(Enum):
    MUSIC_RNN = 'music_rnn'
    TRANSFORMER = 'transformer'


class EnumType(click.Choice):
    """Case-insensitive enum names, reference composer/click_utils.py:10-82."""

    def __init__(self, enum, case_sensitive=False):
        self._enum = enum
        super().__init__([e.name.lower() for e in enum] + [e.value for e in enum], case_sensitive=case_sensitive)

    def convert(self, value, param, ctx):
        if isinstance(value, self._enum):
            return value
        v = super().convert(value, param, ctx).lower()
        for e in self._enum:
            if v in (e.name.lower(), str(e.value).lower()):
                return e
        self.fail('invalid choice: %s' % value, param, ctx)


def get_default_config():
    return Path(__file__).parent / 'default_config.yml'


def _require_transformer(model_type):
    if model_type != ModelType.TRANSFORMER:
        logging.error('Only the transformer model type is implemented on MI355X (the MusicRNN is outside the hot path).')
        sys.exit(1)


def _runtime(config):
    rt = config.transformer.get('runtime', None) or {}
    return rt.get('dtype', 'bf16'), int(rt.get('seed', 0))


def _vocab(config):
    d = config.dataset
    return ds.vocab_size(d.time_step_increment, d.max_time_steps, d.velocity_bins)


def create_model(model_type, config, **kwargs):
    """cli.py:95-141: positional constructor arguments in the reference's order."""
    _require_transformer(model_type)
    m = config.transformer.model
    dtype, seed = _runtime(config)
    vocab = _vocab(config)
    model = Transformer(
        vocab, m.embedding_size, m.window_size, m.decoder_layers_count, m.attention_head_count,
        m.use_relative_attention, m.initializer_mean, m.initializer_stddev, m.attention_dropout_rate,
        m.residual_dropout_rate, m.layer_normalization_epsilon, m.scale_attention, m.use_layer_normalization,
        dtype=kwargs.get('dtype', dtype), seed=seed, max_batch=kwargs.get('max_batch', config.transformer.train.batch_size),
        max_seq=m.window_size)
    return model, vocab


def get_dataset(model_type, dataset_path, config, mode='', max_files=None, shuffle_files=True, shuffle_dataset=True,
                rank=0, world_size=1, seed=0):
    """cli.py:185-276: a directory dataset (`<root>/{train,test}/**/*.data`) or an exported `.tfrecord` file."""
    if mode not in ('train', 'test', ''):
        raise ValueError('\'{}\' is an invalid dataset mode! Must be one of: \'train\', \'test\', or none.'.format(mode))
    p = Path(dataset_path)
    if not p.is_dir():
        if not p.is_file() or p.suffix != '.tfrecord':                                   # cli.py:232-241
            logging.error('\'{}\' is an invalid dataset path! The dataset can either be a directory of processed MIDI '
                          'files or a TFRecord file.'.format(p))
            sys.exit(1)
        dataset, header = tfrecord.load_tfrecord_dataset(p, shuffle=shuffle_dataset, seed=seed, rank=rank, world_size=world_size)
        warning = 'The TFRecord file was probably exported using a different config.'    # cli.py:246-268
        if header['model_type'] != model_type.value:
            logging.warning('Model type mismatch when loading \'{}\'. Expected {} but found {}. {}'.format(
                p, model_type.value, header['model_type'], warning))
            click.confirm('Do you want to continue? This may cause errors or corrupt the training session.', abort=True)
        for name, want in (('batch', config.transformer.train.batch_size), ('window', config.transformer.model.window_size)):
            if header[name + '_size'] != want:
                logging.error('Expected a {} size of {} but found {}. {}'.format(name, want, header[name + '_size'], warning))
                sys.exit(1)
        return dataset
    p = p / mode
    if not p.exists():
        logging.error('Could not get {} dataset since \'{}\' has no {} folder.'.format(mode, dataset_path, mode))
        sys.exit(1)
    files = ds.get_processed_files(p)
    if shuffle_files:
        np.random.default_rng(seed).shuffle(files)          # cli.py:229-230 (np.random.shuffle, unseeded there)
    if max_files is not None:
        files = files[:max_files]
    d = config.dataset
    return ds.load_dataset(files, config.transformer.train.batch_size, config.transformer.model.window_size,
                           shuffle=shuffle_dataset, seed=seed, rank=rank, world_size=world_size,
                           expect_settings=(d.time_step_increment, d.max_time_steps, d.velocity_bins))


def _train_options(clip_norm=0.0, accumulate_steps=1, warmup_steps=0, source='transformer.train'):
    try:
        return check_train_options(clip_norm, accumulate_steps, warmup_steps)
    except (ValueError, TypeError) as e:
        raise click.UsageError('{}: {}'.format(source, e))


def train_options_from(config, clip_norm=None, accumulate_steps=None, warmup_steps=None):
    """(clip_norm, accumulate_steps, warmup_steps): the optional keys of `transformer.train` (absent in the reference's files: off),
    overridden by the flags that were given; a bad value is a click.UsageError."""
    t = config.transformer.train
    pick = lambda flag, key, default: t.get(key, default) if flag is None else flag
    return _train_options(pick(clip_norm, 'clip_norm', 0.0), pick(accumulate_steps, 'accumulate_steps', 1),
                          pick(warmup_steps, 'warmup_steps', 0))


def _augment_options(augment_transpose=0, augment_stretch=0.0, random_crop=False, source='transformer.train'):
    try:
        return check_augment_options(augment_transpose, augment_stretch, random_crop)
    except (ValueError, TypeError) as e:
        raise click.UsageError('{}: {}'.format(source, e))


def augment_options_from(config, augment_transpose=None, augment_stretch=None, random_crop=None):
    """(augment_transpose, augment_stretch, random_crop): the optional keys of `transformer.train` (absent in the reference's files:
    off), overridden by the flags that were given; a bad value is a click.UsageError."""
    t = config.transformer.train
    pick = lambda flag, key, default: t.get(key, default) if flag is None else flag
    return _augment_options(pick(augment_transpose, 'augment_transpose', 0), pick(augment_stretch, 'augment_stretch', 0.0),
                            pick(random_crop, 'random_crop', False))


def _eval_options(eval_freq=0, eval_max_windows=None, early_stop_patience=0, keep_best=False, source='transformer.train'):
    try:
        return check_eval_options(eval_freq, eval_max_windows, early_stop_patience, keep_best)
    except (ValueError, TypeError) as e:
        raise click.UsageError('{}: {}'.format(source, e))


def eval_options_from(config, eval_freq=None, eval_split=None, eval_max_windows=None, early_stop_patience=None, keep_best_checkpoint=None):
    """(eval_freq, eval_split, eval_max_windows, early_stop_patience, keep_best): the optional keys of `transformer.train` (absent in
    the reference's files: off, split 'test'), overridden by the flags that were given; a bad value is a click.UsageError."""
    t = config.transformer.train
    pick = lambda flag, key, default: t.get(key, default) if flag is None else flag
    freq, windows, patience, keep = _eval_options(pick(eval_freq, 'eval_freq', 0), pick(eval_max_windows, 'eval_max_windows', None),
                                                  pick(early_stop_patience, 'early_stop_patience', 0),
                                                  pick(keep_best_checkpoint, 'keep_best_checkpoint', False))
    split = str(pick(eval_split, 'eval_split', 'test'))
    if not split or '/' in split or split in ('.', '..'):
        raise click.UsageError('transformer.train: eval_split \'{}\' must name a folder of the dataset path'.format(split))
    return freq, split, windows, patience, keep


def get_eval_stream(dataset_path, config, split='test', max_files=None):
    """The id stream of a held-out split of a directory dataset (uint16, files in sorted order), read against the config's settings
    like the train split.  No device use; what cannot be validated on is a click.UsageError."""
    p = Path(dataset_path)
    if not p.is_dir():
        raise click.UsageError('--eval-freq needs a directory dataset with a \'{}\' folder: \'{}\' holds pre-cut batches (or does not '
                               'exist)'.format(split, dataset_path))
    files = ds.get_processed_files(p / split) if (p / split).is_dir() else []
    if not files:
        raise click.UsageError('--eval-split {}: \'{}\' is missing or holds no .data file'.format(split, p / split))
    if max_files is not None:
        files = files[:max_files]
    d = config.dataset
    try:
        ids = ds.read_id_stream(files, expect_settings=(d.time_step_increment, d.max_time_steps, d.velocity_bins))
    except ValueError as e:
        raise click.UsageError(str(e))
    need = config.transformer.model.window_size + 1
    if len(ids) < need:
        raise click.UsageError('--eval-split {}: \'{}\' holds {} events, one window needs window_size + 1 = {}'.format(
            split, p / split, len(ids), need))
    return ids


def event_class_ranges(config):
    """{class name: range of ids} of the config's vocabulary, in id order: the classes of `score --by-event-type`."""
    d = config.dataset
    rg = ds.event_ranges(ds.event_value_ranges(d.time_step_increment, d.max_time_steps, d.velocity_bins))
    return collections.OrderedDict((EVENT_TYPE_NAMES[t], r) for t, r in rg.items())


def get_device_dataset(dataset_path, config, augment, max_files=None, rank=0, world_size=1, seed=0):
    """The train split of a directory dataset as a DeviceDataset: the files and their order are get_dataset's, the batches are built
    on the device (augment = (transpose, stretch, random_crop))."""
    from composer_amd import grammar as gm
    p = Path(dataset_path) / 'train'
    if not p.exists():
        logging.error('Could not get train dataset since \'{}\' has no train folder.'.format(dataset_path))
        sys.exit(1)
    files = ds.get_processed_files(p)
    np.random.default_rng(seed).shuffle(files)
    if max_files is not None:
        files = files[:max_files]
    d = config.dataset
    settings = (d.time_step_increment, d.max_time_steps, d.velocity_bins)
    transpose, stretch, random_crop = augment
    return ds.DeviceDataset(ds.read_id_stream(files, expect_settings=settings), config.transformer.train.batch_size,
                            config.transformer.model.window_size, gm.EventGrammar.from_dataset_params(*settings, rules=0), shuffle=True,
                            seed=seed, rank=rank, world_size=world_size, random_crop=random_crop, transpose=transpose, stretch=stretch)


def get_config_from_restoredir(restoredir):
    """cli.py:500-514"""
    path = Path(restoredir) / 'config.yml'
    if not path.exists():
        logging.error('Failed to restore model from \'{}\'! Could not find \'config.yml\' file!'.format(restoredir))
        sys.exit(1)
    return cfgmod.get(path)


def _init_distributed(model):
    """One process per GPU under torch.distributed.run: gloo for the bootstrap, RCCL (inside the library) for gradients."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if not dist.is_initialized():
            dist.init_process_group('gloo', rank=rank, world_size=world)
        uid = [Transformer.new_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        model.init_data_parallel(rank, world, uid[0])
    return rank, world


@click.group()
@click.option('--verbosity', '-v', default='info', help='Logging level name.')
def cli(verbosity):
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        # Library load order: a data-parallel job uses torch.distributed (gloo) to hand the RCCL id to the ranks, so
        # torch comes into this process anyway -- import it BEFORE libcomposer_hip.so is loaded, so that the dynamic linker binds the
        # library to the HIP runtime and the RCCL torch has already mapped: one runtime, the RCCL bench.py and the tests run on.
        import torch.distributed  # noqa: F401
    logging.basicConfig(level=getattr(logging, str(verbosity).upper(), logging.INFO), format='%(levelname)s: %(message)s')


@cli.command('make-config')
@click.argument('filepath', default='config.yml')
def make_config(filepath):
    """Creates a configuration file from the default configuration (cli.py:69-78)."""
    shutil.copy(get_default_config(), filepath)
    logging.info('Created configuration file \'{}\'.'.format(filepath))


@cli.command()
@click.argument('model-type', type=EnumType(ModelType, False))
@click.option('-c', '--config', 'config_filepath', default=None)
def summary(model_type, config_filepath):
    """Prints the parameter table of the model (cli.py:424-440)."""
    config = cfgmod.get(config_filepath or get_default_config())
    model, _ = create_model(model_type, config)
    model.summary()


@cli.command()
@click.argument('model-type', type=EnumType(ModelType, False))
@click.argument('dataset-path')
@click.option('--logdir', default='./output/logdir/', help='The root log directory. Defaults to \'./output/logdir\'.')
@click.option('--restoredir', default=None, type=str, help='The directory of the model to continue training.')
@click.option('-c', '--config', 'config_filepath', default=None)
@click.option('-e', '--epochs', 'epochs', default=10, help='The number of epochs to train for. Defaults to 10.')
@click.option('--use-generator/--no-use-generator', default=False, help='Accepted for compatibility; datasets are memory-mapped ids either way.')
@click.option('--max-files', default=None, type=int)
@click.option('--save-freq-mode', 'save_frequency_mode', type=EnumType(ModelSaveFrequencyMode, False), default='global_step')
@click.option('--save-freq', 'save_frequency', type=int, default=500)
@click.option('--max-checkpoints', 'max_checkpoints', type=int, default=3)
@click.option('--show-progress-bar/--no-show-progress-bar', 'show_progress_bar', default=True)
@click.option('--max-steps', default=None, type=int, help='Stop after this many steps (not in the reference; for smoke runs).')
@click.option('--checkpoint-format', type=click.Choice(['npz', 'tensorbundle']), default='npz',
              help='npz (default) or the reference\'s TensorBundle files (ckpt-N.index / .data-00000-of-00001). Either is restored.')
@click.option('--clip-norm', default=None, type=float,
              help='Global-norm gradient clipping: 0 off, > 0 clip to this norm, inf measure only (logged as grad_norm). '
                   'Overrides transformer.train.clip_norm.')
@click.option('--accumulate-steps', default=None, type=int,
              help='Micro-batches summed into one optimiser step (steps, --max-steps and --save-freq count optimiser steps). '
                   'Overrides transformer.train.accumulate_steps.')
@click.option('--warmup-steps', default=None, type=int,
              help='Linear learning-rate warm-up over this many optimiser steps (0 off). Overrides transformer.train.warmup_steps.')
@click.option('--augment-transpose', default=None, type=int, metavar='N',
              help='Transpose every training row by a random number of semitones in [-N, N] (0-12; 0 off), on the device. '
                   'Overrides transformer.train.augment_transpose.')
@click.option('--augment-stretch', default=None, type=float, metavar='FRAC',
              help='Stretch the time axis of every training row by a random factor in [1 - FRAC, 1 + FRAC] (0-0.5; 0 off), on the '
                   'device. Overrides transformer.train.augment_stretch.')
@click.option('--random-crop/--no-random-crop', default=None,
              help='Cut training rows at random offsets of the id stream instead of a fixed grid of windows. Overrides '
                   'transformer.train.random_crop.')
@click.option('--eval-freq', default=None, type=int, metavar='N',
              help='Validate on the held-out split every N optimiser steps, on the device: val_loss, val_accuracy and val_nll/<class> '
                   'are logged (0 off). Overrides transformer.train.eval_freq.')
@click.option('--eval-split', default=None, metavar='NAME',
              help='The folder of DATASET-PATH to validate on. Defaults to test. Overrides transformer.train.eval_split.')
@click.option('--eval-max-windows', default=None, type=int, metavar='N',
              help='Validate on the first N windows of the split only. Overrides transformer.train.eval_max_windows.')
@click.option('--early-stop-patience', default=None, type=int, metavar='P',
              help='Stop after P validation passes in a row without a lower val_loss (0 off). Overrides '
                   'transformer.train.early_stop_patience.')
@click.option('--keep-best-checkpoint/--no-keep-best-checkpoint', default=None,
              help='Keep the state with the lowest val_loss so far in <logdir>/best/. Overrides transformer.train.keep_best_checkpoint.')
def train(model_type, dataset_path, logdir, restoredir, config_filepath, epochs, use_generator, max_files,
          save_frequency_mode, save_frequency, max_checkpoints, show_progress_bar, max_steps, checkpoint_format,
          clip_norm, accumulate_steps, warmup_steps, augment_transpose, augment_stretch, random_crop,
          eval_freq, eval_split, eval_max_windows, early_stop_patience, keep_best_checkpoint):
    """Trains the specified model (cli.py:516-589)."""
    _require_transformer(model_type)
    for flag, value in (('--clip-norm', clip_norm), ('--accumulate-steps', accumulate_steps), ('--warmup-steps', warmup_steps)):
        if value is not None:                                    # refused from the arguments, before any device use
            _train_options(**{flag[2:].replace('-', '_'): value}, source=flag)
    for flag, value in (('--augment-transpose', augment_transpose), ('--augment-stretch', augment_stretch)):
        if value is not None:
            _augment_options(**{flag[2:].replace('-', '_'): value}, source=flag)
    for flag, value in (('--eval-freq', eval_freq), ('--eval-max-windows', eval_max_windows),
                        ('--early-stop-patience', early_stop_patience)):
        if value is not None:                                    # (a flag alone: the pairing rule waits for the config's keys)
            _eval_options(**{'eval_freq': 1, flag[2:].replace('-', '_'): value}, source=flag)
    rank = int(os.environ.get('RANK', '0'))
    if restoredir is not None:
        config = get_config_from_restoredir(restoredir)
        model_logdir = None
    else:
        stamp = datetime.datetime.now().strftime('%Y-%m-%d_%H-%M-%S')
        model_logdir = Path(logdir) / '{}-{}'.format(model_type.name.lower(), stamp)
        config = cfgmod.get(config_filepath or get_default_config())
        if rank == 0:
            model_logdir.mkdir(parents=True, exist_ok=True)
            banner = '\n'.join([
                '#########################################################',
                '# Datetime: {}.'.format(datetime.datetime.now()),
                '#########################################################',
                '# This is an autogenerated backup of the configuration file',
                '# used when invoking the train command.',
                '# ',
                '# DO NOT MODIFY THIS FILE!',
                '# Doing so may cause errors upon resuming training.',
                '#########################################################'])
            with open(config.filepath) as src, open(model_logdir / 'config.yml', 'w+') as dst:
                dst.write(banner + '\n' + src.read())
    clip_norm, accumulate_steps, warmup_steps = train_options_from(config, clip_norm, accumulate_steps, warmup_steps)
    augment = augment_options_from(config, augment_transpose, augment_stretch, random_crop)
    if any(augment) and not Path(dataset_path).is_dir():         # refused before any device use
        raise click.UsageError('--augment-transpose / --augment-stretch / --random-crop need a directory dataset: \'{}\' holds '
                               'pre-cut batches (or does not exist)'.format(dataset_path))
    eval_freq, eval_split, eval_max_windows, early_stop_patience, keep_best = eval_options_from(
        config, eval_freq, eval_split, eval_max_windows, early_stop_patience, keep_best_checkpoint)
    eval_ids = get_eval_stream(dataset_path, config, eval_split, max_files) if eval_freq else None     # refused before any device use
    model, _ = create_model(model_type, config)
    rank, world = _init_distributed(model)
    _, seed = _runtime(config)
    eval_dataset, eval_ranges = None, None
    if eval_ids is not None:                                     # the whole split on every rank, in file order: one grid, one verdict
        eval_dataset = ds.DeviceDataset(eval_ids, config.transformer.train.batch_size, config.transformer.model.window_size, shuffle=False)
        eval_ranges = event_class_ranges(config)
    if any(augment):
        dataset = get_device_dataset(dataset_path, config, augment, max_files=max_files, rank=rank, world_size=world, seed=seed)
    else:                                                        # everything off: the host-cut windows, exactly as before
        dataset = get_dataset(model_type, dataset_path, config, 'train', max_files=max_files, rank=rank, world_size=world, seed=seed)
    input_shape = (config.transformer.train.batch_size, config.transformer.model.window_size)
    model.train(dataset, input_shape, model_logdir, restoredir=restoredir, epochs=epochs,
                learning_rate=config.transformer.train.learning_rate, save_frequency_mode=save_frequency_mode,
                save_frequency=save_frequency, max_checkpoints=max_checkpoints,
                show_progress_bar=show_progress_bar and rank == 0, max_steps=max_steps, checkpoint_format=checkpoint_format,
                clip_norm=clip_norm, accumulate_steps=accumulate_steps, warmup_steps=warmup_steps,
                eval_dataset=eval_dataset, eval_freq=eval_freq, eval_max_windows=eval_max_windows,
                early_stop_patience=early_stop_patience, keep_best=keep_best, eval_event_ranges=eval_ranges)
    if rank == 0 and model_logdir is not None:
        click.echo(str(model_logdir))


@cli.command('export-dataset')
@click.argument('model-type', type=EnumType(ModelType, False))
@click.argument('preprocessed-path')
@click.argument('output-path')
@click.option('-c', '--config', 'config_filepath', default=None)
@click.option('--use-generator/--no-use-generator', default=False, help='Accepted for compatibility.')
@click.option('--max-files', default=None, type=int)
def export_dataset(model_type, preprocessed_path, output_path, config_filepath, use_generator, max_files):
    """Exports a processed dataset input pipeline as a TFRecord file (cli.py:346-380): the unshuffled batches of the
    `.data` files under PREPROCESSED-PATH, windowed and batched by the config."""
    _require_transformer(model_type)
    config = cfgmod.get(config_filepath or get_default_config())
    dataset = get_dataset(model_type, preprocessed_path, config, shuffle_dataset=False, max_files=max_files)
    logging.info('Loading dataset and writing to TFRecord. This make take a while...')
    n = tfrecord.export_dataset(dataset, output_path, model_type.value)
    logging.info('Finished exporting \'{}\' as a TFRecord: \'{}\' ({} batches)'.format(preprocessed_path, output_path, n))


@cli.command()
@click.argument('model-type', type=EnumType(ModelType, False))
@click.argument('dataset-path')
@click.argument('restoredir')
@click.option('--use-generator/--no-use-generator', default=False)
@click.option('--max-files', default=None, type=int)
@click.option('--by-event-type', is_flag=True, default=False,
              help='Evaluate ALL windows of the test split in one pass on the device and print the count, mean NLL and accuracy of every '
                   'event class.')
@click.option('--json', 'json_out', default=None, help='With --by-event-type: write the figures to this JSON file.')
def evaluate(model_type, dataset_path, restoredir, use_generator, max_files, by_event_type, json_out):
    """Evaluate the specified model (cli.py:591-615)."""
    config = get_config_from_restoredir(restoredir)
    if json_out is not None and not by_event_type:
        raise click.UsageError('--json needs --by-event-type.')
    if by_event_type:
        _require_transformer(model_type)
        ids = get_eval_stream(dataset_path, config, 'test', max_files)      # refused before any device use
        model, _ = create_model(model_type, config)
        model.load_from_checkpoint(restoredir)
        report = model.evaluate_dataset(ids, event_ranges=event_class_ranges(config))
        click.echo('loss {:.6f} accuracy {:.6f}'.format(report.loss, report.accuracy))
        click.echo('events {} nll {:.9g} bits {:.9g} perplexity {:.9g} top1 {:.9g}'.format(
            report.events, report.loss, report.bits_per_event, report.perplexity, report.accuracy))
        for name, (count, nll, _) in report.by_event_type.items():
            click.echo('  {}: count {} nll {:.9g}'.format(name, count, nll))
        if json_out is not None:
            with open(json_out, 'w') as fh:
                json.dump(report.to_dict(), fh)
        return
    model, _ = create_model(model_type, config)
    model.load_from_checkpoint(restoredir)
    model.compile(config.transformer.train.learning_rate)
    model.build(input_shape=(config.transformer.train.batch_size, None))
    test = get_dataset(model_type, dataset_path, config, 'test', max_files=max_files, shuffle_dataset=False)
    loss, accuracy = model.evaluate(test, verbose=0)
    logging.info('- Finished evaluating model. Loss: {:.4f}, Accuracy: {:.4f}'.format(loss, accuracy))
    click.echo('loss {:.6f} accuracy {:.6f}'.format(loss, accuracy))


@cli.command()
@click.argument('model-type', type=EnumType(ModelType, False))
@click.argument('restoredir')
@click.argument('output-filepath')
@click.option('--prompt', '-p', 'prompt', default=None, help='The path of the MIDI file to prompt the network with.')
@click.option('--prompt-ids', default=None, help='Comma-separated event ids to prompt the network with (instead of --prompt).')
@click.option('--prompt-data', default=None, help='A .data file whose first events prompt the network (instead of --prompt).')
@click.option('--prompt-length', default=10, help='Number of events to take from the start of the prompt. Defaults to 10.')
@click.option('--length', '-l', 'generate_length', default=1024, help='The length of the generated event sequence. Defaults to 1024')
@click.option('--temperature', default=1.0, help='Sampling temperature; 0 = greedy argmax. Defaults to 1.0.')
@click.option('--decode-mode', type=click.Choice(['reference-literal', 'kv-cache', 'kv-slide']), default=None,
              help='kv-cache: model(x, past=presents); reference-literal: the reference\'s loop as written (no past); '
                   'kv-slide: kv-cache that goes on past window_size by re-encoding the last --slide-keep events when the '
                   'window is full (any length). '
                   'Default: kv-cache when prompt + length fits window_size, else reference-literal.')
@click.option('--slide-keep', default=None, type=int,
              help='kv-slide: events kept (re-encoded from position 0) when the window is full, 1 .. window_size - 1. '
                   'Defaults to window_size // 2.')
@click.option('--top-k', default=0, type=int,
              help='Sample from the K most likely events only (ties to the lower id); 0 = off. Defaults to 0.')
@click.option('--top-p', default=1.0, type=float,
              help='Nucleus sampling: sample from the smallest set of most likely events whose probability (after --temperature '
                   'and --top-k) reaches P, in (0, 1]; 1 = off. Defaults to 1.')
@click.option('--constrain/--no-constrain', default=False,
              help='Event-grammar decoding: never sample an event the MIDI conversion would ignore in the current state (a NOTE_OFF of '
                   'a silent pitch, a NOTE_ON of a sounding one, a pedal event that changes nothing). Defaults to off, the '
                   'reference\'s sampler.')
@click.option('--pitch-range', default=None, metavar='LO:HI',
              help='Never sample a NOTE_ON of a pitch outside LO..HI (MIDI pitches, 0 <= LO <= HI <= 127).')
@click.option('--num-samples', default=1, type=click.IntRange(1, 256),
              help='Number of sequences to generate from the prompt, decoded together; sample i uses seed + i and goes to '
                   'OUTPUT-i.mid (or OUTPUT-i.data). Defaults to 1.')
@click.option('--keep-best', default=None, type=int,
              help='Score the --num-samples N sequences under the model (mean log-probability of the generated events, '
                   'temperature 1, no filter) and write only the K best as OUTPUT-0 ... OUTPUT-{K-1}, best first; 1 <= K <= N. '
                   'Defaults to off: every sample is written.')
@click.option('--duration', default=None, type=float, metavar='SECONDS',
              help='Generate SECONDS of music behind the prompt (rounded to the config\'s time step, at least one): the time '
                   'shifts land on it exactly, then every sounding note and the pedal are released, and the sequence ends '
                   'there. --length stays the cap on events (a sample that reaches it first is written unfinished); long '
                   'durations want --decode-mode kv-slide, which is not bound to window_size. Defaults to off.')
@click.option('--max-polyphony', default=None, type=int, metavar='N',
              help='Never more than N notes sounding at once (N >= 1): no NOTE_ON is sampled while N pitches sound. '
                   'Defaults to off.')
@click.option('--novelty-against', default=None, metavar='DATASET',
              help='After decoding, match every written sample against the train split of this directory dataset and print, per '
                   'sample, its longest verbatim match, where it lies and the share of the sample covered by matches (the generated '
                   'events only: the prompt is usually taken from a real piece). Defaults to off.')
@click.option('--novelty-min-match', default=None, type=int, metavar='K',
              help='--novelty-against: the shortest run that counts as a match. Defaults to 16.')
@click.option('--novelty-transpose', default=None, type=int, metavar='N',
              help='--novelty-against: also find copies transposed by up to N semitones (0-24). Defaults to 0.')
@click.option('--max-copy', default=None, type=int, metavar='M',
              help='--novelty-against: never extend a verbatim match of prompt + sample with the train split past M events (1-64; '
                   'copies transposed by up to --novelty-transpose semitones count): the event that would is not sampled. TIME_SHIFT '
                   'events are exempt. Defaults to off.')
def generate(model_type, restoredir, output_filepath, prompt, prompt_ids, prompt_data, prompt_length, generate_length,
             temperature, decode_mode, slide_keep, top_k, top_p, constrain, pitch_range, num_samples, keep_best, duration,
             max_polyphony, novelty_against, novelty_min_match, novelty_transpose, max_copy):
    """Generate a MIDI file (cli.py:617-680): MIDI prompt -> event ids -> model -> event ids -> MIDI.  An output path
    ending in `.data` gets the event ids in the dataset's binary format instead of a MIDI file.  With --num-samples N > 1
    the N sequences are decoded as one batch and written to OUTPUT-0 ... OUTPUT-{N-1} (same suffix); --top-k / --top-p apply
    to every sample, and so do --constrain / --pitch-range, --duration and --max-polyphony."""
    from composer_amd import notes as nt
    from composer_amd import grammar as gm
    if max_copy is not None:                                     # refused from the arguments, before any device use
        from composer_amd import novelty as nv
        if novelty_against is None:
            raise click.UsageError('--max-copy goes with --novelty-against: DATASET is the corpus that must not be copied.')
        if not 1 <= max_copy <= nv.MAX_COPY:
            raise click.UsageError('--max-copy {}: must be in [1, {}].'.format(max_copy, nv.MAX_COPY))
    if novelty_against is None:                                  # refused from the arguments, before any device use
        for flag, value in (('--novelty-min-match', novelty_min_match), ('--novelty-transpose', novelty_transpose)):
            if value is not None:
                raise click.UsageError('{} goes with --novelty-against.'.format(flag))
    else:
        novelty_min_match, novelty_transpose = _novelty_options(16 if novelty_min_match is None else novelty_min_match,
                                                                novelty_transpose or 0, '--novelty-min-match', '--novelty-transpose')
        _novelty_dataset_dir(novelty_against, 'train')
        if not 1 <= generate_length <= 32768:
            raise click.UsageError('--novelty-against: --length {} outside [1, 32768].'.format(generate_length))
    if duration is not None and not (duration > 0 and math.isfinite(duration)):      # refused from the arguments (a NaN fails too)
        raise click.UsageError('--duration {}: SECONDS must be a number > 0.'.format(duration))
    if max_polyphony is not None and max_polyphony < 1:
        raise click.UsageError('--max-polyphony {}: must be >= 1.'.format(max_polyphony))
    if pitch_range is not None:                                  # refused from the arguments, before any device use
        try:
            lo, hi = (int(t) for t in pitch_range.split(':'))
            if not 0 <= lo <= hi <= 127:
                raise ValueError
        except ValueError:
            raise click.UsageError('--pitch-range {}: LO:HI with 0 <= LO <= HI <= 127.'.format(pitch_range))
    if top_k < 0:                                                # refused from the arguments, before any device use
        raise click.UsageError('--top-k {}: must be >= 0 (0 = off).'.format(top_k))
    if not 0.0 < top_p <= 1.0:
        raise click.UsageError('--top-p {}: must be in (0, 1] (1 = off).'.format(top_p))
    if keep_best is not None and not 1 <= keep_best <= num_samples:
        raise click.UsageError('--keep-best {}: must be in [1, --num-samples = {}].'.format(keep_best, num_samples))
    config = get_config_from_restoredir(restoredir)
    x_early = None
    if keep_best is not None:                                    # refused from the arguments and the prompt, before any device use
        x_early = _prompt_ids(prompt, prompt_ids, prompt_data, prompt_length, config.dataset)
        if len(x_early) == 0:                                    # (the scored positions are those behind the prompt: it needs one id)
            raise click.UsageError('--keep-best: the prompt is empty.')
        w = config.transformer.model.window_size
        if len(x_early) + generate_length > w and (decode_mode == 'reference-literal' or
                                                   (decode_mode is None and len(x_early) + generate_length - 1 > w)):
            # that loop draws every id from the whole prefix fed at once, which is not the scoring contract's context
            raise click.UsageError('--keep-best: --decode-mode reference-literal with prompt ({}) + length ({}) > window_size ({}) '
                                   'cannot be scored; use --decode-mode kv-slide.'.format(len(x_early), generate_length, w))
    if slide_keep is not None:                                   # refused from the restored config, before any device use
        if decode_mode != 'kv-slide':
            raise click.UsageError('--slide-keep goes with --decode-mode kv-slide.')
        if not 1 <= slide_keep <= config.transformer.model.window_size - 1:
            raise click.UsageError('--slide-keep {}: must be in [1, window_size - 1 = {}].'.format(
                slide_keep, config.transformer.model.window_size - 1))
    model, _ = create_model(model_type, config, dtype='fp32')
    model.load_from_checkpoint(restoredir)
    model.compile(config.transformer.train.learning_rate)
    model.build(input_shape=(1, None))
    d = config.dataset
    x = x_early if x_early is not None else _prompt_ids(prompt, prompt_ids, prompt_data, prompt_length, d)
    model.reset_states()
    window = config.transformer.model.window_size
    fits = len(x) + generate_length - 1 <= window
    if decode_mode == 'kv-cache' and not fits:
        # position ids would run past the wpe table (transformer.py:675-679,786): an explicit request cannot be honoured, and
        # silently switching modes would change what is sampled (context-conditioned vs the reference's context-free loop)
        raise click.UsageError('--decode-mode kv-cache: prompt ({}) + length ({}) - 1 exceeds window_size ({}); at most '
                               '--length {} fits, or use --decode-mode reference-literal.'.format(
                                   len(x), generate_length, window, window - len(x) + 1))
    if decode_mode is None:
        # no mode asked for: the KV cache when it fits; otherwise the reference's own loop, which never feeds `past` back
        # (cli.py:663-676) and can therefore emit any length -- said on stderr whatever the log level
        decode_mode = 'kv-cache' if fits else 'reference-literal'
        if not fits:
            click.echo('composer generate: prompt ({}) + length ({}) - 1 exceeds window_size ({}); using the reference\'s '
                       'decode loop (--decode-mode reference-literal). With the KV cache at most --length {} fits.'.format(
                           len(x), generate_length, window, window - len(x) + 1), err=True)
    click.echo('decode-mode: {}'.format(decode_mode), err=True)
    click.echo('sampling: temperature {} top-k {} top-p {}'.format(
        temperature, top_k if top_k else 'off', top_p if top_p < 1.0 else 'off'), err=True)
    out = Path(output_filepath)
    out.parent.mkdir(parents=True, exist_ok=True)
    slide = {'slide_keep': slide_keep} if decode_mode == 'kv-slide' else {}
    if top_k or top_p < 1.0:
        slide.update(top_k=top_k, top_p=top_p)
    if constrain or pitch_range is not None:
        # the layout always (the pitch range is stated in it); the dynamic rules only with --constrain
        g = gm.EventGrammar.from_dataset_params(d.time_step_increment, d.max_time_steps, d.velocity_bins,
                                                rules=gm.ALL if constrain else 0)
        slide.update(grammar=g)
        if pitch_range is not None:
            slide.update(banned_ids=g.pitch_range_bans(lo, hi))
        click.echo('grammar: constrain {} pitch-range {}'.format('on' if constrain else 'off', pitch_range or 'off'), err=True)
    timed = None
    if duration is not None or max_polyphony is not None:
        # the budget reads the layout (which ids shift time, which are notes): supplied with no rule when nothing above gave it
        g = slide.get('grammar') or gm.EventGrammar.from_dataset_params(d.time_step_increment, d.max_time_steps, d.velocity_bins,
                                                                        rules=0)
        steps = max(1, int(round(duration * 1000.0 / d.time_step_increment))) if duration is not None else None
        slide.update(grammar=g, duration_steps=steps, max_polyphony=max_polyphony or 0)
        timed = gm.TimedRules(g, steps or 0, max_polyphony or 0)
        click.echo('budget: duration {} max-polyphony {}'.format(
            '{} steps of {} ms'.format(steps, d.time_step_increment) if steps else 'off', max_polyphony or 'off'), err=True)

    def report(i, ids):                                          # one line per sample: what was written, and whether it ended
        if timed is None or not timed.time_steps:
            return
        st = timed.fold(x, ids)
        click.echo('sample {}: {} events, {:.3f} s, finished {}'.format(
            i, len(ids), (st.g.time_steps - (st.t_end - timed.time_steps)) * d.time_step_increment / 1000.0,
            'yes' if st.done_at >= 0 else 'no'), err=True)
    guard_corpus = None
    if max_copy is not None:
        # the corpus goes to the device before the decode: every draw is checked against it (cmp_decode_copy_guard)
        guard_corpus = open_novelty_corpus(novelty_against, config, 'train')
        slide.update(copy_guard=guard_corpus.guard(max_copy, transpose=novelty_transpose))
        click.echo('copy-guard: max-copy {} transpose {} against {} events'.format(max_copy, novelty_transpose, len(guard_corpus.ids)),
                   err=True)

    def guard_report(batched, n):                                # one line per decoded sample: the columns the rule took away
        if guard_corpus is not None:
            for i in range(n):
                click.echo('copy-guard: sample {} banned_columns {}'.format(i, model.decode_copy_guard_state(batched, i)), err=True)

    def novelty_report(samples):                                 # one line per written sample, from one batched device call
        if novelty_against is None:
            return
        corpus = guard_corpus or open_novelty_corpus(novelty_against, config, 'train')
        for i, r in enumerate(corpus.match([np.asarray(s, np.int32) for s in samples], min_match=novelty_min_match,
                                           transpose=novelty_transpose)):
            click.echo('novelty: sample {} {}'.format(i, r.line()), err=True)
        corpus.close()
    if num_samples == 1 and keep_best is None:
        ids = model.generate(x, generate_length, temperature=temperature, mode=decode_mode, **slide)
        guard_report(False, 1)
        report(0, ids)
        novelty_report([ids])
        _write_generated(list(x) + ids.tolist(), out, d)         # prompt + generated (cli.py:676)
        click.echo(','.join(str(int(i)) for i in ids))
        return
    batch = model.generate_batch([x] * num_samples, generate_length, temperature=temperature, mode=decode_mode, **slide)
    guard_report(True, num_samples)
    if keep_best is not None:
        # prompt ++ ids of every sample under the scoring contract (the run's --slide-keep when it slid); only the generated
        # positions count.  Sample i was drawn with seed + i.
        scores = model.score([list(x) + ids.tolist() for ids in batch], slide_keep=slide_keep if decode_mode == 'kv-slide' else None)
        means = [float(np.mean(s.logp[len(x) - 1:].astype(np.float64))) for s in scores]
        for i, v in enumerate(means):
            click.echo('keep-best: sample {} seed {} mean log-probability {:.6f}'.format(i, model.seed + i, v), err=True)
        order = sorted(range(num_samples), key=lambda i: (-means[i], i))[:keep_best]
        click.echo('keep-best: kept {}'.format(','.join(str(i) for i in order)), err=True)
        batch = [batch[i] for i in order]
    novelty_report(batch)
    for i, ids in enumerate(batch):
        report(i, ids)
        _write_generated(list(x) + ids.tolist(), out.with_name('{}-{}{}'.format(out.stem, i, out.suffix)), d)
        click.echo(','.join(str(int(t)) for t in ids))


def _prompt_ids(prompt, prompt_ids, prompt_data, prompt_length, d):
    """The prompt of `generate` as event ids (host only)."""
    from composer_amd import notes as nt
    if prompt is not None:                                       # cli.py:645-660
        x = nt.prompt_ids_from_midi(prompt, prompt_length, d.time_step_increment, d.max_time_steps, d.velocity_bins)
    elif prompt_ids is not None:
        x = [int(t) for t in prompt_ids.split(',') if t.strip() != '']
    elif prompt_data is not None:
        x = ds.read_data_file(prompt_data)[0].astype(np.int32).tolist()
    else:
        raise NotImplementedError()                              # cli.py:642-643
    return x[:prompt_length]                                     # cli.py:649


EVENT_TYPE_NAMES = {ds.NOTE_ON: 'NOTE_ON', ds.NOTE_OFF: 'NOTE_OFF', ds.VELOCITY: 'VELOCITY', ds.TIME_SHIFT: 'TIME_SHIFT',
                    ds.SUSTAIN_ON: 'SUSTAIN_ON', ds.SUSTAIN_OFF: 'SUSTAIN_OFF'}


def read_score_file(path, d):
    """Event ids of one file to score: `.mid` / `.midi` through the codec path of `generate --prompt` (the whole file), `.data`
    through read_data_file with its settings checked against the config, as load_dataset does."""
    p = Path(path)
    if p.suffix.lower() in ('.mid', '.midi'):
        from composer_amd import notes as nt
        try:
            return nt.prompt_ids_from_midi(p, None, d.time_step_increment, d.max_time_steps, d.velocity_bins)
        except IndexError:                                       # (trim_start of a file without a note)
            raise click.ClickException('{} holds no notes.'.format(p))
    if p.suffix == '.data':
        ids, settings = ds.read_data_file(p)
        want = (d.time_step_increment, d.max_time_steps, d.velocity_bins)
        if tuple(settings) != want:
            raise click.ClickException('{} was preprocessed with {} but the config says {}'.format(p, tuple(settings), want))
        return ids.astype(np.int32).tolist()
    raise click.UsageError('{}: a .mid / .midi or a .data file is expected.'.format(p))


@cli.command()
@click.argument('model-type', type=EnumType(ModelType, False))
@click.argument('restoredir')
@click.argument('files', nargs=-1, required=True)
@click.option('--slide-keep', default=None, type=int,
              help='Events re-encoded from position 0 when a file is longer than window_size (the context rule of generate '
                   '--decode-mode kv-slide), 1 .. window_size - 1. Defaults to window_size // 2.')
@click.option('--by-event-type', is_flag=True, default=False, help='Also print the count and mean NLL of every event class.')
@click.option('--json', 'json_out', default=None, help='Write the figures and the per-event arrays to this JSON file.')
def score(model_type, restoredir, files, slide_keep, by_event_type, json_out):
    """How likely are these pieces under the model?  One line per file: events scored, NLL per event (nats), bits per event,
    perplexity and top-1 accuracy -- every event after the first, each against the context kv-slide generation would draw it
    from (temperature 1, no filter, no grammar)."""
    _require_transformer(model_type)
    config = get_config_from_restoredir(restoredir)
    window = config.transformer.model.window_size
    if slide_keep is not None and not 1 <= slide_keep <= window - 1:     # refused from the restored config, before any device use
        raise click.UsageError('--slide-keep {}: must be in [1, window_size - 1 = {}].'.format(slide_keep, window - 1))
    d = config.dataset
    seqs = [read_score_file(f, d) for f in files]
    for f, s in zip(files, seqs):
        if len(s) == 0:
            raise click.ClickException('{} holds no events.'.format(f))
    model, _ = create_model(model_type, config, dtype='fp32')
    model.load_from_checkpoint(restoredir)
    results = model.score(seqs, slide_keep=slide_keep)
    rg = ds.event_ranges(ds.event_value_ranges(d.time_step_increment, d.max_time_steps, d.velocity_bins))
    report = []
    for f, r in zip(files, results):
        click.echo('{}: events {} nll {:.9g} bits {:.9g} perplexity {:.9g} top1 {:.9g}'.format(
            f, r.events, r.nll_per_event, r.bits_per_event, r.perplexity, r.top1_accuracy))
        entry = dict(file=str(f), **r.to_dict())
        if by_event_type:
            entry['by_event_type'] = {}
            for t, (count, nll) in r.by_event_type(rg).items():
                click.echo('  {}: count {} nll {:.9g}'.format(EVENT_TYPE_NAMES[t], count, nll))
                entry['by_event_type'][EVENT_TYPE_NAMES[t]] = {'count': count, 'nll_per_event': nll}
        report.append(entry)
    if json_out is not None:
        keep = window // 2 if slide_keep is None else slide_keep
        with open(json_out, 'w') as fh:
            json.dump({'window_size': window, 'slide_keep': keep, 'files': report}, fh)


def _novelty_options(min_match, transpose, flag_min_match='--min-match', flag_transpose='--transpose'):
    from composer_amd import novelty as nv
    if min_match < 1:
        raise click.UsageError('{} {}: must be >= 1.'.format(flag_min_match, min_match))
    if not 0 <= transpose <= nv.MAX_TRANSPOSE:
        raise click.UsageError('{} {}: must be in [0, {}].'.format(flag_transpose, transpose, nv.MAX_TRANSPOSE))
    return min_match, transpose


def _novelty_dataset_dir(dataset_path, split):
    p = Path(dataset_path)
    if not p.is_dir() or not (p / split).is_dir():
        raise click.UsageError('\'{}\' is not a directory dataset with a \'{}\' folder: the novelty check reads the pieces of '
                               'a split one by one.'.format(dataset_path, split))
    return p / split


def open_novelty_corpus(dataset_path, config, split='train', max_files=None):
    """The split of a directory dataset as a composer_amd.novelty.Corpus: its files in sorted order, one piece each, named relative to
    the dataset path."""
    from composer_amd import grammar as gm
    from composer_amd import novelty as nv
    root = _novelty_dataset_dir(dataset_path, split)
    files = ds.get_processed_files(root)
    if max_files is not None:
        files = files[:max_files]
    d = config.dataset
    settings = (d.time_step_increment, d.max_time_steps, d.velocity_bins)
    try:
        ids, starts, names = ds.read_id_stream_pieces(files, expect_settings=settings)
    except ValueError as e:
        raise click.ClickException(str(e))
    if len(ids) < 2:
        raise click.ClickException('\'{}\' holds fewer than 2 events.'.format(root))
    vel = ds.event_ranges(ds.event_value_ranges(*settings))[ds.VELOCITY]
    names = [str(Path(f).relative_to(dataset_path)) for f in names]
    return nv.Corpus(ids, starts, names, gm.EventGrammar.from_dataset_params(*settings, rules=0), (vel.start, len(vel)),
                     time_step_ms=d.time_step_increment)


@cli.command()
@click.argument('dataset-path')
@click.argument('files', nargs=-1, required=True)
@click.option('-c', '--config', 'config_filepath', default=None)
@click.option('--restoredir', default=None, type=str, help='Take the configuration from this model directory instead of -c.')
@click.option('--split', default='train', help='The folder of DATASET-PATH to match against. Defaults to train.')
@click.option('--max-files', default=None, type=int)
@click.option('--min-match', default=16, type=int, help='The shortest run that counts as a match. Defaults to 16.')
@click.option('--transpose', default=0, type=int, metavar='N', help='Also find copies transposed by up to N semitones (0-24). Defaults to 0.')
@click.option('--ignore-velocity', is_flag=True, default=False, help='Every VELOCITY event equals every other.')
@click.option('--json', 'json_out', default=None, help='Write the figures and the per-event arrays to this JSON file.')
def novelty(dataset_path, files, config_filepath, restoredir, split, max_files, min_match, transpose, ignore_velocity, json_out):
    """Is this piece new, or a passage of the dataset played back?  For every event of every FILE (.mid / .midi / .data) the longest
    run that occurs verbatim in the split, on the device.  One line per file: events, the longest match in events and seconds, where it
    lies (file, event offset, transposition) and the share of the file covered by matches of at least --min-match events.  A
    time-stretched copy re-chunks its TIME_SHIFT runs and is not found."""
    _novelty_options(min_match, transpose)                       # refused from the arguments, before any device use
    if config_filepath is not None and restoredir is not None:
        raise click.UsageError('-c and --restoredir both name a configuration: give one.')
    _novelty_dataset_dir(dataset_path, split)
    config = get_config_from_restoredir(restoredir) if restoredir is not None else cfgmod.get(config_filepath or get_default_config())
    seqs = [read_score_file(f, config.dataset) for f in files]
    for f, s in zip(files, seqs):
        if len(s) == 0:
            raise click.ClickException('{} holds no events.'.format(f))
        if len(s) > 32768:
            raise click.ClickException('{} holds {} events: at most 32768 per file.'.format(f, len(s)))
    corpus = open_novelty_corpus(dataset_path, config, split, max_files)
    reports = corpus.match(seqs, min_match=min_match, transpose=transpose, ignore_velocity=ignore_velocity)
    corpus.close()
    for f, r in zip(files, reports):
        click.echo('{}: {}'.format(f, r.line()))
    if json_out is not None:
        with open(json_out, 'w') as fh:
            json.dump({'dataset': str(dataset_path), 'split': split, 'min_match': min_match, 'transpose': transpose,
                       'ignore_velocity': bool(ignore_velocity), 'corpus_events': int(len(corpus.ids)),
                       'files': [dict(file=str(f), **r.to_dict()) for f, r in zip(files, reports)]}, fh)


def _write_generated(all_ids, out, d):
    if out.suffix == '.data':
        vr = ds.event_value_ranges(d.time_step_increment, d.max_time_steps, d.velocity_bins)
        rg = ds.event_ranges(vr)
        events = [ds.id_to_event(int(i), rg, vr) for i in all_ids]
        ds.write_data_file(out, events, d.time_step_increment, d.max_time_steps, d.velocity_bins)
    else:                                                        # cli.py:678-680
        from composer_amd import notes as nt
        nt.ids_to_midi(all_ids, out, d.time_step_increment, d.max_time_steps, d.velocity_bins)


if __name__ == '__main__':
    cli()
