"""The reference's ``CompositeAggregationAlgorithm``
(``simulation_lib/algorithm/composite_aggregation_algorithm.py:10-69``): a list of algorithms, of
which the first that takes a round's first message serves the whole round.

Host logic only. Same methods, same assertions: ``process_worker_data`` tries the algorithms in
order until one returns true and then sticks to it (asserting that it keeps taking the round's
messages), ``aggregate_worker_data`` hands the round to it and forgets the choice, and
``NotImplementedError`` is raised when no algorithm takes a message. Every other call goes to every
algorithm.
"""

from __future__ import annotations

from typing import Any

from ..message import Message, ModelParameter
from .aggregation_algorithm import AggregationAlgorithm


class CompositeAggregationAlgorithm(AggregationAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self.__algorithms: list[AggregationAlgorithm] = []
        self.__used_algorithm: AggregationAlgorithm | None = None

    def prepend_algorithm(self, algorithm: AggregationAlgorithm) -> None:
        self.__algorithms.insert(0, algorithm)

    def append_algorithm(self, algorithm: AggregationAlgorithm) -> None:
        self.__algorithms.append(algorithm)

    def set_old_parameter(self, old_parameter: ModelParameter) -> None:
        for algorithm in self.__algorithms:
            algorithm.set_old_parameter(old_parameter=old_parameter)

    def set_config(self, config: Any) -> None:
        for algorithm in self.__algorithms:
            algorithm.set_config(config=config)

    def process_worker_data(self, worker_id: int, worker_data: Message | None) -> bool:
        if self.__used_algorithm is not None:
            res = self.__used_algorithm.process_worker_data(worker_id=worker_id, worker_data=worker_data)
            assert res
            return True
        for algorithm in self.__algorithms:
            if algorithm.process_worker_data(worker_id=worker_id, worker_data=worker_data):
                self.__used_algorithm = algorithm
                return True
        raise NotImplementedError("Failed to process_worker_data")

    def aggregate_worker_data(self) -> Any:
        assert self.__used_algorithm is not None
        res = self.__used_algorithm.aggregate_worker_data()
        self.__used_algorithm = None
        return res

    def clear_worker_data(self) -> None:
        for algorithm in self.__algorithms:
            algorithm.clear_worker_data()

    def exit(self) -> None:
        for algorithm in self.__algorithms:
            algorithm.exit()
