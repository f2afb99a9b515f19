"""
Transition counting for PastML ACR: the file-level front end of marginal_counts / expected_counts (API of
pastml/utilities/transition_counter.py:24-173, without its html visualisation).

Two additions to the reference's interface: ``n_repetitions=None`` (or 0) writes the exact expected counts
(:func:`pastml_amd.ml.expected_counts`) instead of an average over sampled scenarios, and ``column`` may be a list of
columns, ``out_transitions`` then being a template with ``{column}``: all of them go through one ``expected_counts`` call,
i.e. one batch per (number of states, model kind) on the device.
"""
import logging

import pandas as pd

from pastml_amd import PASTML_VERSION
from pastml_amd.acr import calculate_observed_freqs, model2class
from pastml_amd.annotation import ForestStats
from pastml_amd.ml import marginal_counts, expected_counts
from pastml_amd.models import SCALING_FACTOR, SMOOTHING_FACTOR
from pastml_amd.models.CustomRatesModel import CUSTOM_RATES
from pastml_amd.models.EFTModel import EFT
from pastml_amd.models.F81Model import F81
from pastml_amd.models.HKYModel import HKY, HKY_STATES
from pastml_amd.models.JCModel import JC
from pastml_amd.models.JTTModel import JTT, JTT_STATES
from pastml_amd.pipeline import validate_input


def count_transitions(tree, data, column, parameters, out_transitions, data_sep='\t', id_index=0, model=F81,
                      threshold=1, n_repetitions=1000, rate_matrix=None, work_dir=None, html=None, verbose=False,
                      offline=False, colours=None):
    """
    Writes the table of expected numbers of state changes ``from`` (rows) -> to (columns) per ancestral scenario.

    :param tree: path to the input tree(s) in newick format (must be rooted)
    :param data: path to the annotation file (first row: the column names); data_sep, id_index as in the pipeline
    :param column: the annotation column with the character to be analysed -- or a list of columns
    :param parameters: ACR parameters: a path to a parameter file, or {column: path or {param: value}}; with several columns
        a list of paths in the order of the columns, or the dict
    :param out_transitions: path of the output table; with several columns a template containing ``{column}``
    :param model: evolutionary model (one for all columns)
    :param n_repetitions: number of scenarios drawn from the marginal probabilities and averaged over;
        None or 0: the exact expected counts, nothing is drawn
    :param rate_matrix: (CUSTOM_RATES only) path to the rate matrix file, or {column: path}
    :param html, threshold, colours, offline, work_dir: the reference's visualisation; html is not implemented here
    :return: void
    """
    if html:
        raise NotImplementedError('html: the visualisation of the transition counts is PastML\'s own layer; '
                                  'this front end writes the table only')
    if verbose:
        logging.basicConfig(level=logging.DEBUG, format='%(asctime)s: %(message)s', datefmt='%H:%M:%S')
    logger = logging.getLogger('pastml')

    several = not isinstance(column, str)
    given = list(column) if several else [column]
    if several:
        if '{column}' not in out_transitions:
            raise ValueError('With several columns out_transitions must be a template containing {column}.')
        if isinstance(parameters, str):
            raise ValueError('With several columns the parameters must be given per column (a list or a dict).')
    elif not isinstance(parameters, dict):
        parameters = [parameters]
    if rate_matrix is not None and not isinstance(rate_matrix, (dict, list)):
        rate_matrix = [rate_matrix] * len(given)

    forest, columns, column2states, parameters, rates = \
        validate_input(tree, given, data, data_sep, id_index, parameters=parameters, rates=rate_matrix)

    forest_stats = ForestStats(forest)
    models = []
    for col in columns:
        states = column2states[col]
        if model in {HKY, JTT}:
            initial_states = states
            states = HKY_STATES if HKY == model else JTT_STATES
            if not set(initial_states) & set(states):
                raise ValueError('The allowed states for model {} are {}, '
                                 'but your annotation file specifies {} as states in column {}.'
                                 .format(model, ', '.join(states), ', '.join(initial_states), col))
        _, observed_frequencies, _ = calculate_observed_freqs(col, forest, states)
        models.append(model2class[model](parameter_file=parameters.get(col), rate_matrix_file=rates.get(col),
                                         reoptimise=False, states=states, forest_stats=forest_stats,
                                         observed_frequencies=observed_frequencies))
        # states the model does not know leave the annotations (pastml/utilities/transition_counter.py:141-150)
        state_set = set(states)
        for root in forest:
            for n in root.traverse():
                if hasattr(n, col):
                    n.add_feature(col, state_set & getattr(n, col))

    exact = not n_repetitions
    logger.debug('\n=============COUNTING TRANSITIONS for {} ({})==============================='
                 .format(', '.join(columns), 'exact' if exact else '{} repetitions'.format(n_repetitions)))
    for m in models:
        logger.debug(m)
    if exact:
        results = expected_counts(forest, columns, models)
    else:
        results = [marginal_counts(forest, col, m, n_repetitions=n_repetitions) for col, m in zip(columns, models)]
    for col, m, result in zip(columns, models, results):
        out = out_transitions.format(column=col) if several else out_transitions
        pd.DataFrame(data=result, columns=m.states, index=m.states).to_csv(out, sep='\t', index_label='from')
        logger.info('Transition counts are saved as {}.'.format(out))


def main():
    """
    Entry point, calling :py:func:`pastml_amd.utilities.transition_counter.count_transitions` with command-line arguments.

    :return: void
    """
    import argparse

    parser = argparse.ArgumentParser(description="Transition counting for PastML ACR", prog='transition_counter')

    tree_group = parser.add_argument_group('tree-related arguments')
    tree_group.add_argument('-t', '--tree', help="input tree(s) in newick format (must be rooted).",
                            type=str, required=True)

    annotation_group = parser.add_argument_group('annotation-file-related arguments')
    annotation_group.add_argument('-d', '--data', required=False, type=str, default=None,
                                  help="annotation file in tab/csv format with the first row containing the column names. "
                                       "If not given, the annotations should be contained in the tree file itself.")
    annotation_group.add_argument('-s', '--data_sep', required=False, type=str, default='\t',
                                  help="column separator for the annotation table (tab by default, ',' for csv).")
    annotation_group.add_argument('-i', '--id_index', required=False, type=int, default=0,
                                  help="index of the annotation table column containing tree tip names (0 by default).")

    acr_group = parser.add_argument_group('ancestral-character-reconstruction-related arguments')
    acr_group.add_argument('-c', '--column', required=True, type=str,
                           help="the name of the annotation table column that contains the character to be analysed.")
    acr_group.add_argument('-m', '--model', default=F81, choices=[JC, F81, EFT, HKY, JTT, CUSTOM_RATES], type=str,
                           required=False, help='evolutionary model.')
    acr_group.add_argument('--parameters', type=str, required=True,
                           help='the ML-method parameters: a tab-delimited file with two columns, parameter names and '
                                '"value" (state frequencies, {}, {}).'.format(SCALING_FACTOR, SMOOTHING_FACTOR))
    acr_group.add_argument('--rate_matrix', type=str, required=False, default=None,
                           help='(only for the {} model) path to the file containing the rate matrix.'.format(CUSTOM_RATES))
    acr_group.add_argument('-n', '--n_repetitions', type=int, required=False, default=1000,
                           help='(default 1000) number of ancestral scenarios drawn from the marginal probabilities and '
                                'averaged over; 0: the exact expected counts, nothing is drawn.')

    out_group = parser.add_argument_group('output-related arguments')
    out_group.add_argument('-o', '--out_transitions', required=True, type=str,
                           help="path to the output transition count file.")
    out_group.add_argument('-v', '--verbose', action='store_true',
                           help="print information on the progress of the analysis (to console)")

    parser.add_argument('--version', action='version', version='%(prog)s {version}'.format(version=PASTML_VERSION))

    params = parser.parse_args()
    count_transitions(**vars(params))


if '__main__' == __name__:
    main()
