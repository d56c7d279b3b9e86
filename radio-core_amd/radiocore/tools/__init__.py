"""Imports all modules from radiocore.tools."""

from radiocore.tools.tuner import *
from radiocore.tools.buffer import *
from radiocore.tools.chopper import *
from radiocore.tools.carrousel import *
from radiocore.tools.ringbuffer import *
from radiocore.tools.sharding import *
from radiocore.tools.wire import *
from radiocore.tools.squelch import *
from radiocore.tools.afc import *
from radiocore.tools.spectrum import *
from radiocore.tools.feeder import *
from radiocore.tools.egress import *
from radiocore.tools.lanes import *
from radiocore.tools.arena import *
from radiocore.tools.tonebank import *
from radiocore.tools.audiofilter import *
from radiocore.tools.blanker import *
from radiocore.tools.gate import *
from radiocore.tools.floor import *
from radiocore.tools.mix import *
from radiocore.tools.busdyn import *
from radiocore.tools import iq, rds, tones, audiofilter
