"""Console entry points ``train <toml>`` / ``infer <toml>`` (cellulus/cli.py:10-27) and the ``measure`` command
(``python -m cellulus_amd.measure <toml> [--contacts] [--topology] [--hull] [--inscribed] [--quantiles 0.25,0.5,0.75] [--mad]
[--texture] [--texture-levels N] [--texture-distance D] [--radial] [--radial-rings N] [--radial-width W] [--radial-wedges]
[--std] [--colocalization] [--coloc-threshold F] [--weighted] [--border-intensity] [--granularity N] [--granularity-background R]
[--granularity-levels L]``) and the ``relate`` command
(``python -m cellulus_amd.relate <toml> --children NAME --parents NAME [--clearance] [--tertiary NAME]``) and the ``expand``
command (``python -m cellulus_amd.expand <toml> --source NAME [--distance D --output NAME] [--neighbours [--limit D]]``) and the
``split`` command (``python -m cellulus_amd.split <toml> --source NAME --output NAME [--depth D] [--edge]``) and the ``fill``
command (``python -m cellulus_amd.fill <toml> --source NAME --output NAME [--max-size N] [--planewise]``) and the ``propagate``
command (``python -m cellulus_amd.propagate <toml> --seeds NAME --output NAME [--mask NAME] [--channel K [--levels 256]]
[--regularisation 1] [--limit COST]``) and the ``skeleton`` command (``python -m cellulus_amd.skeleton <toml> --source NAME
--output NAME [--max-iter N] [--planewise] [--radius] [--prune L] [--graph]``) and the ``granularity`` command (``python -m cellulus_amd.granularity <toml>
--source NAME [--channel K] [--scales 16] [--levels 256] [--background R]``)."""

import click
import tomli

from .configs import ExperimentConfig


def _load(config_file):
    print(f"Reading config from {config_file}")
    with open(config_file, "rb") as f:
        return tomli.load(f)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
def train(config_file):
    from .train import train as train_experiment

    train_experiment(ExperimentConfig(**_load(config_file)))


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
def infer(config_file):
    from .infer import infer as infer_experiment

    infer_experiment(ExperimentConfig(**_load(config_file)))


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--contacts", is_flag=True, help="add the boundary columns and write contacts_bandwidth-<b>.csv")
@click.option("--topology", is_flag=True, help="add the Euler numbers and the Crofton perimeter (2-D) / surface area and sphericity (3-D)")
@click.option("--hull", is_flag=True, help="add the convex hull columns: convex area, solidity, maximum / minimum Feret diameter")
@click.option("--inscribed", is_flag=True, help="add the largest inscribed circle / ball: radius, centre, mean squared distance")
@click.option("--quantiles", default=None, metavar="Q,Q,...",
              help="add per raw channel the intensity quantiles of a comma-separated list in [0, 1], e.g. 0.25,0.5,0.75")
@click.option("--mad", is_flag=True, help="add per raw channel the median absolute deviation of the intensity (unscaled)")
@click.option("--texture", is_flag=True,
              help="add per raw channel Haralick's texture features of the grey-level co-occurrence matrices; the grey levels "
                   "divide the range of the values under each sample's objects")
@click.option("--texture-levels", default=8, show_default=True, metavar="N", type=click.IntRange(2, 32), help="grey levels of --texture")
@click.option("--texture-distance", default=1, show_default=True, metavar="D", type=click.IntRange(1, 64),
              help="pixel distance of the pairs of --texture")
@click.option("--radial", is_flag=True,
              help="add the radial distribution: per ring of every object its area and, per raw channel, its mean, its share of "
                   "the object's intensity and its mean over the object's mean; ring 0 is the rim")
@click.option("--radial-rings", default=4, show_default=True, metavar="N", type=click.IntRange(1, 32), help="rings of --radial")
@click.option("--radial-width", default=None, metavar="W", type=click.IntRange(1, 32768),
              help="rings of --radial that are W pixels wide, counted from the boundary, the last one taking what lies deeper "
                   "[default: rings relative to every object's inscribed radius]")
@click.option("--radial-wedges", is_flag=True,
              help="with --radial (2-D): add per ring the variation of the means of eight 45-degree wedges around the inscribed centre")
@click.option("--std", is_flag=True, help="add per raw channel the (population) standard deviation of the intensity")
@click.option("--colocalization", is_flag=True,
              help="add per pair of raw channels Pearson's correlation, the slope, the overlap coefficient, K1 / K2 and the Manders "
                   "coefficients inside every object (needs at least 2 channels)")
@click.option("--coloc-threshold", default=0.15, show_default=True, metavar="F", type=click.FloatRange(0.0, 1.0),
              help="fraction of an object's maximum from which a pixel counts for the overlap, K1 / K2 and Manders columns")
@click.option("--weighted", is_flag=True,
              help="add per raw channel the integrated intensity, the intensity-weighted centroid and covariance, the distance between "
                   "the plain and the weighted centroid and the position of the brightest pixel")
@click.option("--border-intensity", is_flag=True,
              help="add the number of border pixels of every object and per raw channel the sum, mean, standard deviation, minimum "
                   "and maximum of the intensity over them")
@click.option("--granularity", default=None, metavar="N", type=click.IntRange(1, 64),
              help="add per raw channel the granular spectrum at N scales: the share of the object's intensity that lies in "
                   "bright structure of each size, and what is left")
@click.option("--granularity-background", default=0, show_default=True, metavar="R", type=click.IntRange(0, 64),
              help="with --granularity: remove the background with a top-hat of radius R pixels first; 0: none")
@click.option("--granularity-levels", default=256, show_default=True, metavar="L", type=click.IntRange(2, 65536),
              help="with --granularity: grey levels between the smallest and the largest value of each sample's channel")
def measure(config_file, contacts, topology, hull, inscribed, quantiles, mad, texture, texture_levels, texture_distance, radial,
            radial_rings, radial_width, radial_wedges, std, colocalization, coloc_threshold, weighted, border_intensity, granularity,
            granularity_background, granularity_levels):
    from .measure import measure as measure_experiment

    if quantiles is not None:
        try:
            quantiles = tuple(float(q) for q in quantiles.split(","))
        except ValueError:
            raise click.BadParameter(f"not a comma-separated list of numbers: {quantiles!r}", param_hint="--quantiles")
    measure_experiment(ExperimentConfig(**_load(config_file)).inference_config, contacts=contacts, topology=topology, hull=hull,
                       inscribed=inscribed, quantiles=quantiles, mad=mad, texture=texture, texture_levels=texture_levels,
                       texture_distance=texture_distance, radial=radial, radial_rings=radial_rings, radial_width=radial_width,
                       radial_wedges=radial_wedges, std=std, colocalization=colocalization, coloc_threshold=coloc_threshold,
                       weighted=weighted, border_intensity=border_intensity, granularity=granularity,
                       granularity_background=granularity_background, granularity_levels=granularity_levels)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--children", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects are assigned (the nuclei)")
@click.option("--parents", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects they are assigned to (the cells)")
@click.option("--clearance", is_flag=True,
              help="add how near every child comes to its parent's boundary: distance, position and mean squared depth")
@click.option("--tertiary", default=None, metavar="NAME",
              help="write the parents' maps with every pixel under a child set to 0 (the cytoplasm) into a new dataset NAME")
def relate(config_file, children, parents, clearance, tertiary):
    from .relate import relate_stage

    relate_stage(ExperimentConfig(**_load(config_file)).inference_config, children, parents, clearance=clearance, tertiary=tertiary)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--source", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects are grown (the nuclei)")
@click.option("--distance", default=None, metavar="D", type=click.FloatRange(0.0),
              help="grow every object by D pixels (Euclidean, inclusive) without letting neighbours merge; needs --output")
@click.option("--output", default=None, metavar="NAME", help="write the grown objects (the cells) into a new dataset NAME")
@click.option("--neighbours", is_flag=True,
              help="write zones_bandwidth-<b>.csv and zone_pairs_bandwidth-<b>.csv: every object's zone (the pixels nearest to it), "
                   "its reach and its neighbours, touching or not")
@click.option("--limit", default=None, metavar="D", type=click.FloatRange(0.0),
              help="with --neighbours: a zone reaches at most D pixels from its object [default: no limit]")
def expand(config_file, source, distance, output, neighbours, limit):
    from .expand import expand_stage

    expand_stage(ExperimentConfig(**_load(config_file)).inference_config, source, output=output, distance=distance,
                 neighbours=neighbours, limit=limit)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--source", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose touching objects are cut apart")
@click.option("--output", required=True, metavar="NAME", help="write the pieces into a new dataset NAME")
@click.option("--depth", default=1.0, show_default=True, metavar="D", type=click.FloatRange(0.0),
              help="merge a basin of the distance map into a higher neighbour where its peak stands less than D pixels above the "
                   "neck between them; 0 keeps every basin")
@click.option("--edge", is_flag=True, help="the image edge counts as background for the distance map")
def split(config_file, source, output, depth, edge):
    from .split import split_stage

    split_stage(ExperimentConfig(**_load(config_file)).inference_config, source, output, depth=depth, edge=edge)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--source", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects' holes are closed")
@click.option("--output", required=True, metavar="NAME", help="write the repaired objects into a new dataset NAME")
@click.option("--max-size", default=None, metavar="N", type=click.IntRange(0),
              help="leave holes of more than N pixels open; 0 fills nothing and only lists the holes [default: no cap]")
@click.option("--planewise", is_flag=True, help="3-D: fill every slice as a 2-D map of its own (cavities open along z)")
def fill(config_file, source, output, max_size, planewise):
    from .fill import fill_stage

    fill_stage(ExperimentConfig(**_load(config_file)).inference_config, source, output, max_size=max_size, planewise=planewise)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--source", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects are thinned to their centre lines")
@click.option("--output", required=True, metavar="NAME", help="write the skeletons into a new dataset NAME")
@click.option("--max-iter", default=None, metavar="N", type=click.IntRange(0),
              help="stop after N iterations (two sub-iterations each); 0 changes nothing [default: until nothing is deleted]")
@click.option("--planewise", is_flag=True, help="3-D: thin every slice as a 2-D map of its own (3-D maps need it)")
@click.option("--radius", is_flag=True, help="add the smallest, largest and mean squared distance to the object's edge along the skeleton")
@click.option("--prune", default=None, metavar="L", type=click.FloatRange(0.0, 2.0 ** 20 - 2.0 ** -10),    # ceil(L * 1024) < 2^30
              help="remove the spurs (branches from a free end to a junction) shorter than L pixels, in one round [default: none]")
@click.option("--graph", is_flag=True,
              help="add the branch graph's columns (branches, junctions, cycles, spurs, components, branch lengths, longest path) "
                   "and write skeleton_branches_bandwidth-<b>.csv, one row per branch")
def skeleton(config_file, source, output, max_iter, planewise, radius, prune, graph):
    from .skeleton import skeleton_stage

    if prune is not None and prune != prune:                 # (a NaN passes every range check)
        raise click.BadParameter("nan is not a length", param_hint="--prune")
    skeleton_stage(ExperimentConfig(**_load(config_file)).inference_config, source, output, max_iter=max_iter, planewise=planewise,
                   radius=radius, graph=graph, prune=prune)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--source", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects' granular spectra are measured")
@click.option("--channel", default=None, metavar="K", type=click.IntRange(0),
              help="channel of the raw dataset to measure [default: every channel]")
@click.option("--scales", default=16, show_default=True, metavar="N", type=click.IntRange(1, 64),
              help="scales of the spectrum: scale i is a diamond of radius i pixels")
@click.option("--levels", default=256, show_default=True, metavar="L", type=click.IntRange(2, 65536),
              help="grey levels between the smallest and the largest value of each sample's channel")
@click.option("--background", default=0, show_default=True, metavar="R", type=click.IntRange(0, 64),
              help="remove the background with a top-hat of radius R pixels first; 0: none")
def granularity(config_file, source, channel, scales, levels, background):
    from .granularity import granularity_stage

    granularity_stage(ExperimentConfig(**_load(config_file)).inference_config, source, channel=channel, scales=scales, levels=levels,
                      background=background)


@click.command()
@click.argument("config_file", type=click.Path(exists=True))
@click.option("--seeds", required=True, metavar="NAME",
              help="label dataset of the segmentation container whose objects are grown (the nuclei)")
@click.option("--output", required=True, metavar="NAME", help="write the territories into a new dataset NAME")
@click.option("--mask", default=None, metavar="NAME",
              help="dataset of the segmentation container whose non-zero pixels the seeds may grow into [default: everywhere]")
@click.option("--channel", default=None, metavar="K", type=click.IntRange(0),
              help="channel of the raw dataset that guides the growth: a step costs the difference in grey levels [default: flat]")
@click.option("--levels", default=256, show_default=True, metavar="N", type=click.IntRange(2, 65536),
              help="with --channel: grey levels between the smallest and the largest value under the mask and the seeds")
@click.option("--regularisation", default=1, show_default=True, metavar="R", type=click.IntRange(0, 65535),
              help="price of distance: a step costs R times 3, 4 or 5 (face, edge, corner) plus the difference in grey levels")
@click.option("--limit", default=None, metavar="COST", type=click.IntRange(0, 2 ** 30 - 1),
              help="a territory reaches no pixel whose cheapest path costs more than COST [default: no limit]")
def propagate(config_file, seeds, output, mask, channel, levels, regularisation, limit):
    from .propagate import propagate_stage

    propagate_stage(ExperimentConfig(**_load(config_file)).inference_config, seeds, output, mask=mask, channel=channel, levels=levels,
                    regularisation=regularisation, limit=limit)
