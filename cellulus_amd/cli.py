"""Console entry points ``train <toml>`` / ``infer <toml>`` (cellulus/cli.py:10-27) and the ``measure`` command
(``python -m cellulus_amd.measure <toml> [--contacts] [--topology] [--hull] [--inscribed]``)."""

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
def measure(config_file, contacts, topology, hull, inscribed):
    from .measure import measure as measure_experiment

    measure_experiment(ExperimentConfig(**_load(config_file)).inference_config, contacts=contacts, topology=topology, hull=hull,
                       inscribed=inscribed)
