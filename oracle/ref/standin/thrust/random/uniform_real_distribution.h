#pragma once
#include <thrust/random.h>
